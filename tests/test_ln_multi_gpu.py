"""tc_layernorm_fwd_multi (include/transception_bridge.h): several independent LayerNorm (+ GELU) forwards in one launch, against one
tc_layernorm_fwd call per segment on the same inputs.  Each segment runs the kernel body and the lane-group shape the single call picks for
its width, so y, mean and rstd are compared as bit patterns; outputs are larger than needed and pre-filled with a sentinel, and the whole
buffers are compared.  Segments with the interleaved statistics (rstd == mean + 1: the layout Graph.mixffn uses) stand beside plain ones."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from transception_amd._lib import ACT_GELU, ACT_NONE, LN_MULTI_MAX, TC_BF16, TC_F16, TC_F32, TcError, TcLnSeg, lib  # noqa: E402
from transception_amd.seeded_init import seeded_tensor  # noqa: E402

DEV = "cuda:0"
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
SENT = -96.0
SHAPES = [(5, 1280), (3, 2048), (7, 64), (2, 512)]                 # (rows, C): 5, 8, 1 and 2 quads of four channels per lane
#        segments (indices into SHAPES)   interleaved statistics per segment
CASES = [((0, 1),       (True, True)),                             # the two wide MixFFN sites of a bridge layer
         ((1, 0),       (False, True)),
         ((2, 3),       (False, False)),
         ((0, 1, 2),    (True, False, True)),
         ((3, 2, 1, 0), (True, True, False, False)),
         ((0, 0),       (False, True))]                            # the same shape twice


def _name(dtype):
    return str(dtype).split(".")[-1]


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def vals(tag, shape, dtype, scale=3.0):
    return torch.from_numpy(seeded_tensor("ln_multi/" + tag, shape, scale)).to(dtype).to(DEV)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(bits(got), bits(want))


class Seg:
    def __init__(self, tag, rows, Cc, inter, dtype):
        self.rows, self.C, self.inter = rows, Cc, inter
        self.ldx, self.ldy = Cc + 8, Cc + 16
        self.x = vals(tag + "x", (rows, self.ldx), dtype)
        self.gamma, self.beta = vals(tag + "g", (Cc,), dtype, 1.0) + 1.0, vals(tag + "b", (Cc,), dtype, 0.5)
        self.dtype = dtype

    def outputs(self):
        y = torch.full((self.rows + 2, self.ldy), SENT, dtype=self.dtype, device=DEV)
        if self.inter:
            stat = torch.full((self.rows + 3, 2), SENT, dtype=torch.float32, device=DEV)
            return y, stat, stat.data_ptr(), stat.data_ptr() + 4
        mean, rstd = (torch.full((self.rows + 3,), SENT, dtype=torch.float32, device=DEV) for _ in range(2))
        return y, (mean, rstd), mean.data_ptr(), rstd.data_ptr()


def run(segs, act, dt, multi):
    L, s = lib(), stream()
    outs = [g.outputs() for g in segs]
    if multi:
        arr = (TcLnSeg * len(segs))(*[TcLnSeg(g.x.data_ptr(), g.gamma.data_ptr(), g.beta.data_ptr(), o[0].data_ptr(), o[2], o[3], g.ldx, g.ldy,
                                              g.rows, g.C, 1e-5, act) for g, o in zip(segs, outs)])
        L.tc_layernorm_fwd_multi(arr, len(segs), dt, s)
    else:
        for g, o in zip(segs, outs):
            L.tc_layernorm_fwd(g.x.data_ptr(), g.ldx, g.gamma.data_ptr(), g.beta.data_ptr(), o[0].data_ptr(), g.ldy, o[2], o[3], g.rows, g.C,
                               1e-5, act, 1, 0, dt, s)
    torch.cuda.synchronize()
    return outs


def check(segs, got, want):
    for g, a, b in zip(segs, got, want):
        assert same_bits(a[0], b[0]), (g.rows, g.C)
        assert bool((b[0][:g.rows, :g.C] != SENT).any()) and bool((b[0][g.rows:] == SENT).all()) and bool((b[0][:, g.C:] == SENT).all())
        if g.inter:
            assert same_bits(a[1], b[1]) and bool((b[1][:g.rows] != SENT).all()) and bool((b[1][g.rows:] == SENT).all())
        else:
            assert same_bits(a[1][0], b[1][0]) and same_bits(a[1][1], b[1][1]) and bool((b[1][1][g.rows:] == SENT).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=_name)
@pytest.mark.parametrize("act", [ACT_NONE, ACT_GELU], ids=["plain", "gelu"])
@pytest.mark.parametrize("case", CASES, ids=str)
def test_multi_equals_one_call_per_segment(case, act, dtype):
    which, inter = case
    assert 2 <= len(which) <= LN_MULTI_MAX
    segs = [Seg(f"{case}{k}", *SHAPES[i], inter[k], dtype) for k, i in enumerate(which)]
    check(segs, run(segs, act, TC[dtype], True), run(segs, act, TC[dtype], False))


@pytest.mark.parametrize("dtype,shapes", [(torch.float32, [(5, 1280), (7, 64)]),              # fp32 storage
                                          (torch.bfloat16, [(4100, 64), (3, 2048)]),          # a segment of 4096 rows or more
                                          (torch.float16, [(2, 512)])],                       # one segment
                         ids=["f32", "rows4100", "single"])
def test_segments_outside_the_one_launch_form_fall_back(dtype, shapes):
    """The entry then issues the per-segment launches itself: the same results."""
    segs = [Seg(f"fb{k}{_name(dtype)}", r, c, k == 0, dtype) for k, (r, c) in enumerate(shapes)]
    check(segs, run(segs, ACT_GELU, TC[dtype], True), run(segs, ACT_GELU, TC[dtype], False))


def test_refusals_launch_nothing():
    L, s = lib(), stream()
    segs = [Seg("ref0", 5, 1280, True, torch.bfloat16), Seg("ref1", 3, 2048, False, torch.bfloat16)]
    outs = [g.outputs() for g in segs]

    def arr(**bad):
        a = (TcLnSeg * 2)(*[TcLnSeg(g.x.data_ptr(), g.gamma.data_ptr(), g.beta.data_ptr(), o[0].data_ptr(), o[2], o[3], g.ldx, g.ldy, g.rows, g.C,
                                    1e-5, ACT_GELU) for g, o in zip(segs, outs)])
        for k, v in bad.items():
            setattr(a[1], k, v)                                    # the SECOND segment is the bad one: the first must not have run
        return a

    for bad in (dict(C=2050), dict(C=4096), dict(rows=0), dict(ldx=2049), dict(act=1), dict(x=None), dict(rstd=None)):
        with pytest.raises(TcError, match="status -1"):
            L.tc_layernorm_fwd_multi(arr(**bad), 2, TC_BF16, s)
    for n, dt in ((0, TC_BF16), (LN_MULTI_MAX + 1, TC_BF16), (2, 7)):
        with pytest.raises(TcError, match="status -1"):
            L.tc_layernorm_fwd_multi(arr(), n, dt, s)
    torch.cuda.synchronize()
    assert all(bool((o[0] == SENT).all()) for o in outs)
