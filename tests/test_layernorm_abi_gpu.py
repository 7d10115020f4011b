"""Every dispatch path of the LayerNorm family of csrc/norm.hip on the C ABI -- tc_layernorm_fwd, tc_layernorm_ps_fwd, tc_layernorm_bwd,
tc_layernorm_ps_bwd, tc_layernorm_bwd_params, tc_layernorm_bwd_defer, tc_layernorm_fold and the two query functions, called through
transception_amd._lib on raw pointers in float32, bfloat16 and float16, against the float64 model of tests/ln_ref.py.  DESIGN.md ("LayerNorm
dispatch: branches and the tests that reach them") lists each branch, its condition and the test below that reaches it.

What is exact is compared bit for bit on whole buffers: the mean of power-of-two rows, dbeta without activation (through atomics, the two-level
fold, parked partials + tc_layernorm_fold, and ln_param_grad_kernel), tc_layernorm_fold on synthetic partials, and everything a call must not
write -- inputs (NaN outside the logical operand), sentinels, an unusable workspace, the arrival counters of a usable one.  rstd, y, dx and
dgamma are held elementwise by the bounds ln_ref derives (tests/test_ln_ref_host.py shows that honest fp32 arithmetic stays inside them and
that a list of mistakes does not); 16-bit outputs add half a storage spacing.  The backward is given the float64 statistics rounded once.

Alignment: a kernel is only called with operands aligned to its own access width; the misaligned cases are those the host dispatch itself
routes to the 4-wide kernels."""
import ctypes as C

import pytest
import torch

import ln_ref as R

pytestmark = pytest.mark.gpu

from transception_amd._lib import TC_BF16, TC_F16, TC_F32, TcError, TcLnFold, lib  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
ids = lambda d: str(d).split(".")[-1]  # noqa: E731
EACH_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=ids)
EACH_HALF = pytest.mark.parametrize("dtype", HALF, ids=ids)
REJECT = dict(match="status -1")                                           # TC_ERR_ARG
WS_FLOATS = 4096 + 3 * 1024 * 2 * 512                                      # counters + the largest parked set of the cases below
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------- plumbing
def up(t):
    return t.to(DEV)


def addr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def sync():
    torch.cuda.synchronize()


def exact(got, want64, what=""):
    """got == the float64 reference cast to got's type, on the whole buffer; the reference itself must be a float32 value."""
    assert R.is_f32_value(want64), "the test's own inputs must make the fp32 result exact: " + what
    g, want = got.detach().cpu(), want64.to(got.dtype)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    if not torch.equal(g, want):
        bad = (g != want).nonzero()
        i = tuple(bad[0].tolist())
        pytest.fail(f"{what}: {bad.shape[0]} of {g.numel()} elements differ, first at {i}: got {float(g[i])}, want {float(want[i])}")


def same_bits(got, want, what=""):
    g = got.detach().cpu().contiguous()
    assert g.dtype == want.dtype and g.shape == want.shape, what
    iv = {4: torch.int32, 2: torch.int16, 1: torch.uint8}[g.element_size()]
    assert torch.equal(g.view(iv), want.contiguous().view(iv)), what


def within(got, want64, bound, dtype, what):
    """|got - want64| <= bound (+ half a storage spacing of a 16-bit type) at every element."""
    e = R.excess(got, want64, bound, dtype)
    if not float(e.max()) <= 0:
        i = tuple((e == e.max()).nonzero()[0].tolist())
        pytest.fail(f"{what}: {int((e > 0).sum())} of {e.numel()} elements outside their bound, worst at {i}: got {float(got[i])}, want "
                    f"{float(want64[i])}, bound {float(bound[i]):.3e}, over by {float(e[i]):.3e}")


def close(got_dev, m, want64, bound, what):
    """The operand's place in the buffer within its bound, every other element of the buffer as it was."""
    g = got_dev.detach().cpu()
    within(m.logical(g), want64.reshape(m.rows, m.C), bound.reshape(m.rows, m.C), g.dtype, what)
    rest = g.clone()
    m.logical(rest).copy_(m.logical())
    same_bits(rest, m.flat, what + ": outside the operand")


def close_params(got_dev, p0, want64, bound, what):
    """A += target [groups] blocks pstride apart: the blocks within their bound of start + want64, the sentinels around them kept."""
    g = got_dev.detach().cpu()
    b = torch.zeros_like(p0.flat, dtype=torch.float64)
    for i in range(p0.groups):
        b[i * p0.wstride:i * p0.wstride + p0.n] = bound.reshape(p0.groups, -1)[i]
    within(g, p0.expect_add(want64.reshape(p0.groups, -1)), b, F32, what)


def ready(o):
    """The premise of a case, asserted once per storage type (tests/test_ln_ref_host.py asserts all of them without a device)."""
    if not o.__dict__.get("_ready"):
        assert o.premise()
        o._ready = True
    return o


def ops(name, dtype):
    return ready(R.CASES[name].on(dtype))


_HOST = {"x": lambda o: o.x, "dy": lambda o: o.dy, "res": lambda o: o.res, "gamma": lambda o: o.gamma, "beta": lambda o: o.beta}


def D(o, name):
    """Device copy of an input (uploaded once; nothing may write to it: `untouched`)."""
    d = o.__dict__.setdefault("_dev", {})
    if name not in d:
        d[name] = up(_HOST[name](o).flat)
    return d[name]


def A(o, name):
    return addr(D(o, name), getattr(_HOST[name](o), "lead", 0))


def untouched(o):
    for name, t in o.__dict__.get("_dev", {}).items():
        same_bits(t, _HOST[name](o).flat, f"{o.tag}: {name} is only read")


def release(name):
    """Drop the operands, references and device copies of a many-row case."""
    R.CASES[name]._built.clear()
    torch.cuda.empty_cache()


_ws = None


def ws():
    """The TcGemm.ws-style workspace: 16 KiB of arrival counters, zero before and after every launch, then room for the parked partials."""
    global _ws
    if _ws is None:
        _ws = torch.zeros(4 * WS_FLOATS + 16, dtype=torch.uint8, device=DEV)
    return _ws


def ws_args(o, form):
    """(scratch, scratch_floats, check()) of the four workspace forms of a backward launch with parameter gradients."""
    c = o.c
    if form == "null":                                                     # no workspace -> plain atomics
        return None, 0, lambda: None
    w, need = ws(), R.scratch_floats(c.C, c.groups, R.bwd_nblk(c.rows, c.C))
    if form == "ws":                                                       # usable -> parked partials, arrival counters, two-level fold
        assert need <= WS_FLOATS and need <= int(lib().tc_layernorm_bwd_scratch_floats(c.rows, c.C, c.groups))

        def zero():
            assert int(w[:16384].count_nonzero()) == 0, f"{o.tag}: the arrival counters must be zero again"
        return addr(w), WS_FLOATS, zero
    before = w.clone()
    keep = lambda: same_bits(w, before.cpu(), f"{o.tag}: an unusable workspace is not written")  # noqa: E731
    if form == "small":                                                    # one float short of counters + partials: legal, unusable -> atomics
        return addr(w), need - 1, keep
    assert form == "unaligned"                                             # large enough, 4 bytes off the 16-byte grid -> atomics
    return addr(w, 4), WS_FLOATS, keep


def stat_buf(n, vals=None):
    t = torch.full((n + 2,), R.SENT if vals is None else R.NAN, dtype=F32)
    if vals is not None:
        t[:n] = vals
    return t


# ---------------------------------------------------------------------------------------------------------------- one entry, one call, whole buffers
def run_fwd(o, inter=False):
    """tc_layernorm_fwd / tc_layernorm_ps_fwd: y within its bound on the whole buffer, mean exact (power-of-two C) or bounded, rstd bounded; inter:
    the statistics as [rows][2] pairs, selected by rstd == mean + 1."""
    c = o.c
    tot = c.groups * c.rows
    y0 = o.y0()
    yd = up(y0.flat)
    if inter:
        st = up(stat_buf(2 * tot))
        pm, pr = addr(st), addr(st, 1)
    else:
        md, rd = up(stat_buf(tot)), up(stat_buf(tot))
        pm, pr = addr(md), addr(rd)
    if c.ps is None:
        lib().tc_layernorm_fwd(A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(yd), c.ld["y"], pm, pr, c.rows, c.C, c.eps, c.act, c.groups,
                               c.pstride, TC[o.dtype], stream())
    else:
        lib().tc_layernorm_ps_fwd(A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(yd), c.ld["y"], pm, pr, *c.ps, c.C, c.eps, TC[o.dtype],
                                  stream())
    sync()
    if inter:
        s = st.cpu()
        mean, rstd, tail = s[0:2 * tot:2], s[1:2 * tot:2], s[2 * tot:]
    else:
        mean, rstd, tail = md.cpu()[:tot], rd.cpu()[:tot], torch.cat([md.cpu()[tot:], rd.cpu()[tot:]])
    wy, wm, wr = o.ref_fwd()
    by, bm, br = o.bound_fwd()
    assert bool((tail == R.SENT).all()), f"{o.tag}: the statistics end at groups * rows"
    if c.C & (c.C - 1) == 0:
        exact(mean, wm, f"{o.tag}: mean")
    else:
        within(mean, wm, bm, F32, f"{o.tag}: mean")
    within(rstd, wr, br, F32, f"{o.tag}: rstd")
    close(yd, y0, wy, by, f"{o.tag}: y")
    untouched(o)


def run_bwd(o, params=True, res=None, form="null", defer=False, entry="bwd"):
    """tc_layernorm_bwd / _ps_bwd / _bwd_defer (+ tc_layernorm_fold) / _bwd_params on the float64 statistics rounded once: dx within its bound on the
    whole buffer, dgamma within its bound and dbeta exact (bounded behind a GELU) on their whole += targets.  res: None, "sep" (rows of their own)
    or "alias" (dres == dx, ldres == lddx: the rows dx replaces).  Returns dx as the device holds it."""
    c = o.c
    tot, G = c.groups * c.rows, c.groups
    m32, r32 = o.stats32()
    md, rd = up(stat_buf(tot, m32)), up(stat_buf(tot, r32))
    dx0 = o.dx0()
    if res == "alias":
        dx0.logical().copy_(o.res.logical())
    dxd = up(dx0.flat)
    pres, ldres = (addr(dxd), dx0.ld) if res == "alias" else ((A(o, "res"), c.ld["res"]) if res == "sep" else (None, 0))
    dg0, db0 = o.dg0(), o.db0()
    dgd, dbd = up(dg0.flat), up(db0.flat)
    pg, pb = (addr(dgd), addr(dbd)) if params else (None, None)
    dt, part, nf = TC[o.dtype], None, 0
    if entry == "params":
        lib().tc_layernorm_bwd_params(A(o, "dy"), c.ld["dy"], A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(md), addr(rd), pg, pb, c.rows, c.C,
                                      c.act, G, c.pstride, dt, stream())
        check = lambda: None  # noqa: E731
    elif c.ps is not None:
        wsp, wsf, check = ws_args(o, form)
        lib().tc_layernorm_ps_bwd(A(o, "dy"), c.ld["dy"], A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(md), addr(rd), addr(dxd), dx0.ld, pg, pb,
                                  *c.ps, c.C, wsp, wsf, dt, stream())
    elif defer:
        nblk = int(lib().tc_layernorm_bwd_nblk(c.rows, c.C))
        assert nblk == R.bwd_nblk(c.rows, c.C, True, True) and nblk > 0
        nf = G * nblk * 2 * c.C
        part = torch.full((nf + 2,), R.NAN, dtype=F32, device=DEV)
        lib().tc_layernorm_bwd_defer(A(o, "dy"), c.ld["dy"], A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(md), addr(rd), addr(dxd), dx0.ld,
                                     pres, ldres, pg, pb, c.rows, c.C, c.act, G, c.pstride, addr(part), nf, dt, stream())
        check = lambda: None  # noqa: E731
    else:
        wsp, wsf, check = ws_args(o, form) if params else (None, 0, lambda: None)
        lib().tc_layernorm_bwd(A(o, "dy"), c.ld["dy"], A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(md), addr(rd), addr(dxd), dx0.ld, pres,
                               ldres, pg, pb, c.rows, c.C, c.act, G, c.pstride, wsp, wsf, dt, stream())
    sync()
    wdx, wdg, wdb = o.ref_bwd(res is not None)
    bdx, bdg, bdb = o.bound_bwd(res is not None, dg0, db0)
    what = f"{o.tag}: params={params} res={res} ws={form} defer={defer} {entry}"
    if entry == "params":
        same_bits(dxd, dx0.flat, what + ": dx is not this entry's")
    else:
        close(dxd, dx0, wdx, bdx, what + ": dx")
    if defer:
        same_bits(dgd, dg0.flat, what + ": dgamma waits for the fold")
        same_bits(dbd, db0.flat, what + ": dbeta waits for the fold")
        assert bool(part[nf:].isnan().all()) and not bool(part[:nf].isnan().any()), what + ": every workgroup parks exactly its 2 C floats"
        site = TcLnFold()
        site.part, site.dgamma, site.dbeta, site.pstride, site.nblk, site.C, site.groups = addr(part), addr(dgd), addr(dbd), c.pstride, nblk, c.C, G
        lib().tc_layernorm_fold(C.byref(site), 1, stream())
        sync()
    if not params:
        same_bits(dgd, dg0.flat, what + ": no dgamma asked for")
        same_bits(dbd, db0.flat, what + ": no dbeta asked for")
    else:
        close_params(dgd, dg0, wdg, bdg, what + ": dgamma")
        if c.act == R.ACT_NONE:
            exact(dbd, db0.expect_add(wdb.reshape(G, -1)), what + ": dbeta")
        else:
            close_params(dbd, db0, wdb, bdb, what + ": dbeta")
    same_bits(md, stat_buf(tot, m32), what + ": mean is only read")
    same_bits(rd, stat_buf(tot, r32), what + ": rstd is only read")
    check()
    untouched(o)
    return dxd


# ---------------------------------------------------------------------------------------------------------------- forward
@EACH_DTYPE
@pytest.mark.parametrize("Cc", R.WIDTHS + R.PARTIAL)
def test_fwd_width_classes(Cc, dtype):
    """ln_fwd_kernel (fp32) / ln_fwd_kernel16 (16-bit) <GS, NV, 1> of TC_LN_DISPATCH: C = 64 / 128 / 256 / 320 / 1024 / 1280 / 2048 are the seven
    (lane group, pieces per lane) classes, C = 4 / 36 / 160 leave lane groups of the first three partly filled; rows = 37 < 4096 is ragged
    against every rows-per-block value.  ldy != ldx, both larger than C, x behind a shifted base."""
    o = ops(f"w{Cc}", dtype)
    assert R.lane_group(Cc) == {64: (16, 1), 128: (32, 1), 256: (64, 1), 320: (64, 2), 1024: (64, 4), 1280: (64, 5), 2048: (64, 8), 4: (16, 1),
                                36: (16, 1), 160: (64, 1)}[Cc]
    assert o.c.ld["x"] != o.c.ld["y"] and min(o.c.ld["x"], o.c.ld["y"]) > Cc
    run_fwd(o)


@EACH_DTYPE
@pytest.mark.parametrize("name", ["eps025", "offset", "const"])
def test_fwd_inputs_that_expose_the_statistics(name, dtype):
    """The same <16, 1, 1> kernels on the inputs that tell mistakes apart: eps = 0.25 (an eps omitted or outside the root), rows offset by 512 /
    1021.5 / 125.5 (a one-pass variance cancels), constant rows (variance 0: y = beta, rstd = eps^-1/2)."""
    run_fwd(ops(name, dtype))


@EACH_DTYPE
@pytest.mark.parametrize("name", ["inflight4", "inflight2"])
def test_fwd_rows_in_flight(name, dtype):
    """rows = 4099 >= 4096: the <GS, NV, RPT> instantiations with RPT = 4 (NV = 1: C = 64) and RPT = 2 (NV = 2: C = 320) rows per lane group in
    flight; 4099 leaves a group of rows with one live row, whose others re-read the last row and store nothing."""
    o = ops(name, dtype)
    assert o.c.rows >= 4096 and R.lane_group(o.c.C)[1] == (1 if name == "inflight4" else 2)
    run_fwd(o)
    release(name)


@pytest.mark.parametrize("name,dtype", [("big64", torch.bfloat16), ("big64", torch.float16), ("big128", torch.bfloat16), ("big256", torch.float16),
                                        ("big512", torch.bfloat16)], ids=lambda v: v if isinstance(v, str) else ids(v))
def test_fwd_v8_kernel(name, dtype):
    """ln_fwd_v8_kernel<T, C / 8, 4>: 16-bit storage, C in {64, 128, 256, 512}, no activation, every row piece 16-byte aligned (ld % 8 == 0, aligned
    bases) and rows = 65541 >= 65536; 65541 = 4 * 16385 + 1 leaves one live row in the last group of four."""
    o = ops(name, dtype)
    c = o.c
    assert c.rows >= 65536 and c.C in R.V8_CS and not (c.ld["x"] | c.ld["y"]) & 7 and c.lead % 8 == 0
    run_fwd(o)
    if name == "big64":
        run_fwd(o, inter=True)                                                # the [rows][2] statistics of the 8-wide kernel
    release(name)


@EACH_HALF
@pytest.mark.parametrize("name", ["big64m1", "big64ldx4"])
def test_fwd_beside_the_v8_kernel(name, dtype):
    """The C = 64 problem of test_fwd_v8_kernel where the dispatch keeps ln_fwd_kernel16<16, 1, 4>: one row short of 65536, and 65541 rows with
    ldx = C + 4 (rows off the 16-byte grid).  The same bounds hold on either side of the threshold."""
    o = ops(name, dtype)
    assert o.c.rows < 65536 or o.c.ld["x"] & 7
    run_fwd(o)
    release(name)


@EACH_DTYPE
@pytest.mark.parametrize("name", ["g3p8", "g3p4", "g2w1280", "g2c36"])
def test_fwd_groups(name, dtype):
    """blockIdx.y = group: stacked row blocks, parameters pstride apart with NaN between the blocks; pstride = C + 8 and C + 4 (the latter fails the
    8-wide alignment test, which only matters from 65536 rows: test_fwd_v8_groups_interleaved), separate and interleaved statistics (offsets
    g rows sst)."""
    o = ops(name, dtype)
    assert o.c.groups > 1 and o.c.pstride > o.c.C and bool(o.gamma.flat[o.c.C:o.c.pstride].isnan().all())
    run_fwd(o)
    run_fwd(o, inter=True)


def test_fwd_v8_groups_interleaved():
    """ln_fwd_v8_kernel with groups = 2 (pstride = C + 8) and the [groups rows][2] statistics: 65537 rows per group."""
    o = ops("big64g2", torch.bfloat16)
    assert o.c.rows >= 65536 and o.c.pstride % 8 == 0
    run_fwd(o, inter=True)
    release("big64g2")


@EACH_DTYPE
def test_fwd_interleaved_statistics(dtype):
    """rstd == mean + 1 -> sst = 2 on the 4-wide kernels (37 and 4099 rows)."""
    run_fwd(ops("w64", dtype), inter=True)
    run_fwd(ops("w1280", dtype), inter=True)
    run_fwd(ops("inflight4", dtype), inter=True)
    release("inflight4")


@EACH_DTYPE
@pytest.mark.parametrize("name", ["gelu64", "gelu1280", "gelu36"])
def test_fwd_gelu(name, dtype):
    """act == TC_ACT_GELU: gelu_f (fp32, Abramowitz-Stegun) / gelu_poly (16-bit) behind the affine map, inside ln_ref's PHI_ERR figures."""
    run_fwd(ops(name, dtype))


@EACH_DTYPE
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("Cc", [64, 96])
def test_ps_fwd(Cc, p, dtype):
    """tc_layernorm_ps_fwd: LnMap{p, H, W} with B = 2, H = 3, W = 5, ldx = p p C + 8 > p p C: output pixel (b, h p + p1, w p + p2) reads chunk
    p1 p + p2 of source row (b, h, w)."""
    o = ops(f"ps{p}c{Cc}", dtype)
    assert o.c.ld["x"] > p * p * Cc
    run_fwd(o)


# ---------------------------------------------------------------------------------------------------------------- backward
@EACH_DTYPE
@pytest.mark.parametrize("Cc", R.WIDTHS + R.PARTIAL + (512,))
def test_bwd_width_classes(Cc, dtype):
    """ln_bwd_kernel<T, GS, NV, 1> in the seven classes and the three partly filled lane groups at rows = 37, strided dy and dx, plain atomics
    (scratch NULL); 16-bit C = 64 / 128 / 256 / 512 are ln_bwd_v8_kernel<T, C / 8, 1>; C = 1280 / 2048 with parameter gradients is the wide split
    (dx-only ln_bwd_kernel<64, 5 / 8, 1>, then ln_param_grad_kernel)."""
    o = ops(f"w{Cc}", dtype)
    assert o.c.ld["dy"] != o.c.ld["dx"] and min(o.c.ld["dy"], o.c.ld["dx"]) > Cc
    run_bwd(o)


@EACH_DTYPE
@pytest.mark.parametrize("name", ["eps025", "offset", "const"])
def test_bwd_inputs_that_expose_the_statistics(name, dtype):
    """The backward on the eps = 0.25, offset and constant rows (xh = 0: dgamma = 0, dx = rstd (a - mean a))."""
    run_bwd(ops(name, dtype))


@EACH_DTYPE
def test_bwd_row_pairing(dtype):
    """ln_bwd_kernel<T, 16, 1, 2>: NV == 1 and rows = 8197 >= 8192, 257 workgroups (fp32; 16-bit with ldx = C + 4, since aligned 16-bit rows of 64 are
    the 8-wide kernel's)."""
    name = "ilp" if dtype == F32 else "ilpldx4"
    o = ops(name, dtype)
    assert o.c.rows >= 8192 and R.bwd_nblk(o.c.rows, 64) == 257 and (dtype == F32 or o.c.ld["x"] & 7)
    run_bwd(o, form="ws")
    run_bwd(o, params=False)
    release(name)


@pytest.mark.parametrize("rpt", [2, 4])
@pytest.mark.parametrize("Cc", R.V8_CS)
def test_bwd_v8_rows_in_flight(Cc, rpt):
    """ln_bwd_v8_kernel<T, C / 8, 2 / 4> (1: test_bwd_width_classes): the row counts come from ln_ref.v8_rows -- the host's rule
    rows >= rpt * nblk * 2048 / C -- with nblk restated in ln_ref.bwd_nblk and held to tc_layernorm_bwd_nblk where the two are the same function
    (the deferred form; a launch that folds at its tail caps at 1024 workgroups).  rows = 2^k + 5: a ragged tail for 2 and 4 rows in flight."""
    name = f"v8c{Cc}r{rpt}"
    c = R.CASES[name]
    o = ops(name, R.case_dtypes(c)[0])
    assert int(lib().tc_layernorm_bwd_nblk(c.rows, Cc)) == R.bwd_nblk(c.rows, Cc, True, True)
    nblk = R.bwd_nblk(c.rows, Cc, True, False)
    assert R.v8_rows_in_flight(c.rows, Cc, nblk) == rpt
    assert c.rows % rpt and R.scratch_floats(Cc, 1, nblk) <= int(lib().tc_layernorm_bwd_scratch_floats(c.rows, Cc, 1))
    run_bwd(o, form="ws")
    release(name)


def test_bwd_v8_deferred_rows_in_flight():
    """The deferred launch of the same kernel, whose nblk IS the query's: C = 512 at the first 2^k + 5 rows for which the host's rule gives 2 rows in
    flight with tc_layernorm_bwd_nblk workgroups."""
    rows = next(r for r in (2 ** k + 5 for k in range(8, 16)) if R.v8_rows_in_flight(r, 512, int(lib().tc_layernorm_bwd_nblk(r, 512))) == 2)
    assert rows == R.CASES["v8c512r4"].rows                                   # 16389: four rows in flight at 1024 workgroups, two at 1025
    o = ops("v8c512r4", R.case_dtypes(R.CASES["v8c512r4"])[0])
    run_bwd(o, defer=True)
    release("v8c512r4")


@EACH_DTYPE
@pytest.mark.parametrize("name", ["g2w1280", "g2w2048"])
def test_bwd_wide_split(name, dtype):
    """dgamma != NULL, C / 4 > 256, no pixel shuffle: tc_layernorm_bwd re-enters itself for dx (ln_bwd_kernel<64, 5 / 8, 1>, dgamma = NULL) and then
    tc_layernorm_bwd_params (ln_param_grad_kernel) with groups = 2; the workspace is not used; with and without dres."""
    o = ops(name, dtype)
    run_bwd(o, form="ws")
    run_bwd(o, res="alias")


@EACH_DTYPE
def test_bwd_dx_only(dtype):
    """dgamma == dbeta == NULL: the kernels return before the parameter tail (4-wide: fp32 and C = 36; 8-wide: 16-bit C = 64), nothing but dx
    is written."""
    run_bwd(ops("w64", dtype), params=False)
    run_bwd(ops("g2c36", dtype), params=False)
    run_bwd(ops("g3p8", dtype), params=False, res="sep")


@EACH_DTYPE
@pytest.mark.parametrize("res", ["sep", "alias"])
def test_bwd_residual_fan_in(res, dtype):
    """dres != NULL: rows of their own (ldres != lddx), and the engine's form dres == dx with ldres == lddx (each lane reads the piece it replaces);
    4-wide (fp32, C = 36, ldx = C + 4) and 8-wide (16-bit C = 64 / 512) kernels."""
    for name in ("w64", "w512", "g2c36", "inflight4"):
        run_bwd(ops(name, dtype), res=res, form="ws")
    if dtype != F32:
        run_bwd(ops("ldx4", dtype), res=res)
    release("inflight4")


@EACH_DTYPE
@pytest.mark.parametrize("form", ["null", "ws", "small", "unaligned"])
def test_bwd_workspace_forms(form, dtype):
    """ln_bwd_param_tail's three exits from a launch that folds at its tail: scratch NULL, one float short of 4096 + groups nblk 2 C, or 4 bytes off
    the 16-byte grid -> plain atomics, the workspace untouched; usable -> parked rows, arrival counters (left zero), the last of every 8
    workgroups folds.  3 workgroups (one short fold group), 257 (32 full groups and one of 1), 3 groups x 3; dbeta exact in every form."""
    for name in ("w64", "w320", "inflight4", "g3p8", "g3p4"):
        run_bwd(ops(name, dtype), form=form)
    release("inflight4")


@EACH_DTYPE
@pytest.mark.parametrize("name", ["gelu64", "gelu1280", "gelu36"])
def test_bwd_gelu(name, dtype):
    """act == TC_ACT_GELU: dz = dy gelu'(xh gamma + beta) in ln_bwd_kernel (16-bit C = 64 too: the 8-wide kernel has no activation) and, at
    C = 1280, in the wide split's ln_param_grad_kernel; dbeta is bounded here, not exact."""
    run_bwd(ops(name, dtype), form="ws")


@EACH_DTYPE
@pytest.mark.parametrize("name", ["g3p8", "g3p4", "g2c36"])
def test_bwd_groups(name, dtype):
    """Groups with pstride = C + 8 (16-bit: the 8-wide kernel) and C + 4 (pstride % 8 != 0: the 4-wide one): dgamma / dbeta blocks pstride apart, the
    sentinels between and behind them kept."""
    run_bwd(ops(name, dtype))
    run_bwd(ops(name, dtype), form="ws", res="sep")


@EACH_HALF
def test_bwd_misaligned_rows_take_the_4_wide_kernel(dtype):
    """ldx = C + 4 in 16-bit storage: the alignment test of the 8-wide kernel fails and ln_bwd_kernel<T, 16, 1, 1> runs (same bounds)."""
    o = ops("ldx4", dtype)
    assert o.c.ld["x"] & 7
    run_bwd(o, form="ws")


@EACH_DTYPE
@pytest.mark.parametrize("p", [2, 4])
@pytest.mark.parametrize("Cc", [64, 96])
def test_ps_bwd(Cc, p, dtype):
    """tc_layernorm_ps_bwd: x read and dx written through LnMap (lddx = p p C + 16 > p p C), dy by output pixel; with parameter gradients (atomics
    and the in-kernel fold) and without.  16-bit C = 64 is the 8-wide kernel (LnRows8), everything else ln_bwd_kernel."""
    o = ops(f"ps{p}c{Cc}", dtype)
    run_bwd(o)
    run_bwd(o, form="ws")
    run_bwd(o, params=False)


@EACH_DTYPE
@pytest.mark.parametrize("name", ["w36", "g3p8", "g2c36", "g2w1280", "gelu64", "gelu36", "gelu1280"])
def test_bwd_params_alone(name, dtype):
    """tc_layernorm_bwd_params (ln_param_grad_kernel) on its own: C = 36 (one partial 64-column chunk), 64, 1280 (20 chunks), groups 1 / 2 / 3 on
    blockIdx.z, both activations; dx is not its business."""
    run_bwd(ops(name, dtype), entry="params")


# ---------------------------------------------------------------------------------------------------------------- deferred parameter gradients
@EACH_DTYPE
@pytest.mark.parametrize("name", ["w64", "w1024", "g3p4", "gelu36", "inflight4"])
def test_bwd_deferred(name, dtype):
    """tc_layernorm_bwd_defer + tc_layernorm_fold of one site: every workgroup parks its [dgamma C | dbeta C] row (the 8-wide kernel's workgroups
    that own no rows park zeros), dgamma / dbeta wait for the fold; dx is bit-identical to tc_layernorm_bwd's on the same operands."""
    o = ops(name, dtype)
    a = run_bwd(o, defer=True, res="sep")
    b = run_bwd(o, form="ws", res="sep")
    same_bits(a, b.cpu(), f"{o.tag}: dx of the deferred launch == dx of tc_layernorm_bwd")
    if name == "inflight4":
        release(name)


@EACH_DTYPE
def test_fold_three_sites_and_a_shared_target(dtype):
    """One tc_layernorm_fold over three sites of different C and groups (w64, g3p4, g2c36), then one over two sites that name the SAME dgamma /
    dbeta (w64 twice): both contributions land (dbeta exactly twice the column sums)."""
    sites, keep = (TcLnFold * 3)(), []
    os_ = [ops(n, dtype) for n in ("w64", "g3p4", "g2c36")]

    def defer(o, dgd, dbd, site):
        c = o.c
        tot = c.groups * c.rows
        m32, r32 = o.stats32()
        md, rd, dx0 = up(stat_buf(tot, m32)), up(stat_buf(tot, r32)), o.dx0()
        dxd = up(dx0.flat)
        nblk = int(lib().tc_layernorm_bwd_nblk(c.rows, c.C))
        nf = c.groups * nblk * 2 * c.C
        part = torch.full((nf + 2,), R.NAN, dtype=F32, device=DEV)
        lib().tc_layernorm_bwd_defer(A(o, "dy"), c.ld["dy"], A(o, "x"), c.ld["x"], A(o, "gamma"), A(o, "beta"), addr(md), addr(rd), addr(dxd), dx0.ld,
                                     None, 0, addr(dgd), addr(dbd), c.rows, c.C, c.act, c.groups, c.pstride, addr(part), nf, TC[dtype], stream())
        site.part, site.dgamma, site.dbeta, site.pstride, site.nblk, site.C, site.groups = addr(part), addr(dgd), addr(dbd), c.pstride, nblk, c.C, c.groups
        keep.extend([md, rd, dxd, part])
    targets = []
    for i, o in enumerate(os_):
        dg0, db0 = o.dg0(), o.db0()
        dgd, dbd = up(dg0.flat), up(db0.flat)
        defer(o, dgd, dbd, sites[i])
        targets.append((o, dg0, db0, dgd, dbd))
    lib().tc_layernorm_fold(sites, 3, stream())
    sync()
    for o, dg0, db0, dgd, dbd in targets:
        _, wdg, wdb = o.ref_bwd(False)
        _, bdg, _ = o.bound_bwd(False, dg0, db0)
        close_params(dgd, dg0, wdg, bdg, f"{o.tag}: dgamma of a three-site fold")
        exact(dbd, db0.expect_add(wdb.reshape(o.c.groups, -1)), f"{o.tag}: dbeta of a three-site fold")
    o = os_[0]
    dg0, db0 = o.dg0(), o.db0()
    dgd, dbd = up(dg0.flat), up(db0.flat)
    two = (TcLnFold * 2)()
    defer(o, dgd, dbd, two[0])
    defer(o, dgd, dbd, two[1])
    lib().tc_layernorm_fold(two, 2, stream())
    sync()
    twice = lambda t: torch.cat([t, t], 1)                                   # noqa: E731  (two sites on one target: the column sums of 2 x 37 rows)
    _, wdg, wdb = R.bwd(twice(o.dy3()), twice(o.x3()), o.g2(), o.b2(), o.c.eps)
    _, bdg, _ = R.bwd_bounds(twice(o.dy3()), twice(o.x3()), o.g2(), o.b2(), o.c.eps, dg0=dg0.blocks(), db0=db0.blocks())
    close_params(dgd, dg0, wdg, bdg, f"{o.tag}: dgamma named by two sites")
    exact(dbd, db0.expect_add(wdb.reshape(1, -1)), f"{o.tag}: dbeta named by two sites")
    untouched(o)


FOLD_SHAPES = [(n, 36) for n in (1, 3, 4, 29, 32, 33, 128, 129, 4096)] + [(n, 4) for n in (1, 29, 129)] + [(n, 1024) for n in (3, 33, 129)]


def fold_site(tag, nblk, Cc, groups, pstride, site):
    """A synthetic site: grid-valued partials (NaN behind them), grid-valued += targets; returns what the fold must leave, exactly."""
    nf = groups * nblk * 2 * Cc
    part = torch.full((nf + 2,), R.NAN, dtype=F32)
    part[:nf] = R.halves(tag + "/part", (nf,))
    dg0 = R.Params(tag + "/dg0", Cc, groups, pstride, F32, R.halves, R.SENT)
    db0 = R.Params(tag + "/db0", Cc, groups, pstride, F32, R.halves, R.SENT)
    pd, dgd, dbd = up(part), up(dg0.flat), up(db0.flat)
    site.part, site.dgamma, site.dbeta, site.pstride, site.nblk, site.C, site.groups = addr(pd), addr(dgd), addr(dbd), pstride, nblk, Cc, groups
    wdg, wdb = R.fold(part[:nf], nblk, Cc, groups)
    assert (nblk * 2.0 + 2.0) * 2 < 2.0 ** 24                                 # the premise: every partial sum is exact

    def check():
        exact(dgd, dg0.expect_add(wdg), f"{tag}: dgamma")
        exact(dbd, db0.expect_add(wdb), f"{tag}: dbeta")
        same_bits(pd, part, f"{tag}: the partials are only read")
    return check


@pytest.mark.parametrize("nblk,Cc", FOLD_SHAPES)
def test_fold_alone_on_synthetic_partials(nblk, Cc):
    """ln_fold_kernel driven alone: nblk in {1, 3, 4, 29, 32, 33, 128, 129, 4096} straddles the unrolled loop's r + 28 < rend test (a slice of 4
    rows sees 29 -> one batch of eight for slice 0 only, 32 -> one for every slice, 33 -> a batch and a tail) and the 128-row split (129: a second
    range of one row; 4096: 32 ranges); C = 4 and 36 are partial 64-column chunks, C = 1024 is 32 full ones; groups = 2, pstride = C + 4.  The result
    is the float64 sum rounded to fp32, exactly, on the whole dgamma / dbeta buffers."""
    site = TcLnFold()
    check = fold_site(f"fold/{nblk}/{Cc}", nblk, Cc, 2, Cc + 4, site)
    lib().tc_layernorm_fold(C.byref(site), 1, stream())
    sync()
    check()


def test_fold_64_sites():
    """n = 64 = LN_FOLD_SITES sites in one launch: the site search by blk0, sites of different C, nblk and groups."""
    sites = (TcLnFold * 64)()
    checks = [fold_site(f"fold64/{i}", 1 + (i * 7) % 40, (4, 36, 64, 8)[i % 4], 1 + i % 3, 72, sites[i]) for i in range(64)]
    lib().tc_layernorm_fold(sites, 64, stream())
    sync()
    for check in checks:
        check()


# ---------------------------------------------------------------------------------------------------------------- queries
def test_query_functions():
    """tc_layernorm_bwd_nblk: ln_bwd_nblk's deferred, with-parameters value (== ln_ref.bwd_nblk), 0 for C > 1024, C % 4 and rows <= 0;
    tc_layernorm_bwd_scratch_floats: 4096 counter words + 1024 parked rows per group, at least what any launch of the cases parks, 0 for
    no problem at all."""
    L = lib()
    for rows in (1, 15, 16, 17, 37, 4096, 8191, 8192, 16383, 16384, 65541, 262144, 10 ** 6):
        for Cc in (4, 36, 64, 128, 132, 256, 320, 512, 1024):
            assert int(L.tc_layernorm_bwd_nblk(rows, Cc)) == R.bwd_nblk(rows, Cc, True, True), (rows, Cc)
            assert 1 <= R.bwd_nblk(rows, Cc, True, False) <= 1024
    for rows, Cc in ((37, 1028), (37, 1280), (37, 2048), (37, 2052), (37, 62), (0, 64), (-1, 64), (37, 0)):
        assert int(L.tc_layernorm_bwd_nblk(rows, Cc)) == 0, (rows, Cc)
    assert int(L.tc_layernorm_bwd_scratch_floats(37, 64, 3)) == 4096 + 3 * 1024 * 2 * 64
    for c in R.CASES.values():
        if c.C <= 1024:
            need = R.scratch_floats(c.C, c.groups, R.bwd_nblk(c.rows, c.C))
            assert need <= int(L.tc_layernorm_bwd_scratch_floats(c.rows, c.C, c.groups)), c.tag
    for bad in ((0, 64, 1), (37, 0, 1), (37, 64, 0)):
        assert int(L.tc_layernorm_bwd_scratch_floats(*bad)) == 0


# ---------------------------------------------------------------------------------------------------------------- rejections
def test_rejections_write_nothing():
    """Every condition of the entry points' argument tests, one call each, is TC_ERR_ARG before anything is launched: every buffer is compared
    bit for bit afterwards.  tc_layernorm_bwd (unknown act), tc_layernorm_bwd_params (unknown act, C > 2048) and tc_layernorm_fold (C % 4,
    C > 1024 on a site) reject what their siblings reject."""
    L, s = lib(), stream()
    o = ops("w64", F32)
    c, dt = o.c, TC_F32
    tot = c.rows
    m32, r32 = o.stats32()
    bufs = dict(y=o.y0().flat, dx=o.dx0().flat, mean=stat_buf(tot, m32), rstd=stat_buf(tot, r32), dg=o.dg0().flat, db=o.db0().flat,
                part=torch.full((3 * 2 * 64 + 2,), R.NAN, dtype=F32))
    dev = {k: up(v) for k, v in bufs.items()}
    P = {k: addr(v) for k, v in dev.items()}
    x, dy, g, b, ld = A(o, "x"), A(o, "dy"), A(o, "gamma"), A(o, "beta"), c.ld

    def fwd(**kw):
        a = dict(x=x, ldx=ld["x"], g=g, b=b, y=P["y"], ldy=ld["y"], mean=P["mean"], rstd=P["rstd"], rows=c.rows, C=64, eps=c.eps, act=0, groups=1,
                 ps=0, dt=dt)
        a.update(kw)
        with pytest.raises(TcError, **REJECT):
            L.tc_layernorm_fwd(a["x"], a["ldx"], a["g"], a["b"], a["y"], a["ldy"], a["mean"], a["rstd"], a["rows"], a["C"], a["eps"], a["act"],
                               a["groups"], a["ps"], a["dt"], s)

    def bwd(entry="bwd", **kw):
        a = dict(dy=dy, lddy=ld["dy"], x=x, ldx=ld["x"], g=g, b=b, mean=P["mean"], rstd=P["rstd"], dx=P["dx"], lddx=ld["dx"], dres=None, ldres=0,
                 dg=P["dg"], db=P["db"], rows=c.rows, C=64, act=0, groups=1, ps=0, part=P["part"], nf=3 * 2 * 64, dt=dt)
        a.update(kw)
        head = (a["dy"], a["lddy"], a["x"], a["ldx"], a["g"], a["b"], a["mean"], a["rstd"])
        with pytest.raises(TcError, **REJECT):
            if entry == "bwd":
                L.tc_layernorm_bwd(*head, a["dx"], a["lddx"], a["dres"], a["ldres"], a["dg"], a["db"], a["rows"], a["C"], a["act"], a["groups"],
                                   a["ps"], None, 0, a["dt"], s)
            elif entry == "defer":
                L.tc_layernorm_bwd_defer(*head, a["dx"], a["lddx"], a["dres"], a["ldres"], a["dg"], a["db"], a["rows"], a["C"], a["act"], a["groups"],
                                         a["ps"], a["part"], a["nf"], a["dt"], s)
            else:
                L.tc_layernorm_bwd_params(*head, a["dg"], a["db"], a["rows"], a["C"], a["act"], a["groups"], a["ps"], a["dt"], s)

    for k in ("x", "y", "g", "b", "mean", "rstd"):
        fwd(**{k: None})
    for kw in (dict(rows=0), dict(groups=0), dict(C=0), dict(C=62), dict(C=2052), dict(ldx=70), dict(ldy=82), dict(act=1), dict(act=-1), dict(dt=7)):
        fwd(**kw)
    for k in ("dy", "x", "g", "b", "mean", "rstd", "dx", "dg", "db"):         # (dg or db alone NULL: exactly one of the pair)
        bwd(**{k: None})
    for kw in (dict(rows=0), dict(groups=0), dict(C=0), dict(C=62), dict(C=2052), dict(ldx=70), dict(lddy=90), dict(lddx=98),
               dict(dres=P["dx"], ldres=98), dict(act=1), dict(dt=7)):
        bwd(**kw)
    assert int(L.tc_layernorm_bwd_nblk(c.rows, 64)) == 3
    for kw in (dict(part=None), dict(dg=None, db=None), dict(nf=3 * 2 * 64 - 1), dict(C=1028), dict(C=1280), dict(groups=0), dict(act=1), dict(ldx=70)):
        bwd("defer", **kw)
    for k in ("dy", "x", "g", "b", "mean", "rstd", "dg", "db"):
        bwd("params", **{k: None})
    for kw in (dict(rows=0), dict(groups=0), dict(C=62), dict(C=2052), dict(ldx=70), dict(lddy=90), dict(act=1), dict(dt=7)):
        bwd("params", **kw)
    # the pixel-shuffle entries: 2 x 3 x 5 source rows of p p C = 256 columns do not fit the buffers above, which no rejected call touches
    for kw in (dict(B=0), dict(H=0), dict(W=0), dict(p=0), dict(ldx=60), dict(C=62), dict(C=2052)):
        a = dict(B=1, H=1, W=1, p=2, C=16, ldx=64)
        a.update(kw)
        with pytest.raises(TcError, **REJECT):
            L.tc_layernorm_ps_fwd(x, a["ldx"] if "ldx" in kw else 4 * a["C"], g, b, P["y"], ld["y"], P["mean"], P["rstd"], a["B"], a["H"], a["W"],
                                  a["p"], a["C"], c.eps, dt, s)
    for kw in (dict(B=0), dict(p=0), dict(ldx=60), dict(lddx=60), dict(C=1028), dict(dg=None)):
        a = dict(B=1, H=1, W=1, p=2, C=16, ldx=64, lddx=64, dg=P["dg"])
        a.update(kw)
        if "C" in kw:
            a["ldx"] = a["lddx"] = 4 * a["C"]
        with pytest.raises(TcError, **REJECT):
            L.tc_layernorm_ps_bwd(dy, ld["dy"], x, a["ldx"], g, b, P["mean"], P["rstd"], P["dx"], a["lddx"], a["dg"], P["db"], a["B"], a["H"], a["W"],
                                  a["p"], a["C"], None, 0, dt, s)
    # the fold
    def site(**kw):
        t = TcLnFold()
        a = dict(part=P["part"], dgamma=P["dg"], dbeta=P["db"], pstride=0, nblk=3, C=64, groups=1)
        a.update(kw)
        for k, v in a.items():
            setattr(t, k, v)
        return t
    many = (TcLnFold * 65)(*[site() for _ in range(65)])
    with pytest.raises(TcError, **REJECT):
        L.tc_layernorm_fold(None, 1, s)
    for n in (0, -1, 65):
        with pytest.raises(TcError, **REJECT):
            L.tc_layernorm_fold(many, n, s)
    for kw in (dict(part=None), dict(dgamma=None), dict(dbeta=None), dict(nblk=0), dict(C=0), dict(C=62), dict(C=1028), dict(groups=0)):
        two = (TcLnFold * 2)(site(), site(**kw))                              # (a bad second site: nothing of the first is folded either)
        with pytest.raises(TcError, **REJECT):
            L.tc_layernorm_fold(two, 2, s)
    sync()
    for k, v in bufs.items():
        same_bits(dev[k], v, f"a rejected call wrote to {k}")
    untouched(o)
