"""Every dispatch path of csrc/dwconv.hip on the C ABI -- tc_dwconv_fwd, tc_dwconv_bwd_input, tc_dwconv_bwd_weight, tc_dwconv_bwd, tc_dwconv_multi,
tc_ffn_dw_fwd and tc_dw_fold called through transception_amd._lib on raw pointers, in float32, bfloat16 and float16, against the float64
shift-and-add reference of tests/dw_ref.py.  DESIGN.md ("Depthwise dispatch: branches and the tests that reach them") lists each branch, its
condition and the test below that reaches it.

Exactness rule (tests/dw_ref.py, as the GEMM and gate suites): maps are multiples of 1/2 with |v| <= 2, weights and biases multiples of 1/4 with
|v| <= 1, so every product and every fp32 partial sum is exact in any order and a 16-bit output is the float64 result rounded once: the
assertion is got == want64.to(dtype) on the WHOLE buffer -- spare rows, the columns between C and ld, the elements in front of a shifted base
and the sentinel behind the parameter blocks included.  fp32 dw / db are += targets: they start from grid values with sentinels between and
behind the groups' blocks.  Each test first asserts its premise (`ready`: the grids, sum|term| / quantum < 2^24; `exact`: the reference is a
float32 value).  Inputs are NaN outside the logical operand, so one read out of range poisons a result, and are compared bit for bit after
the calls.  The one quantity that cannot be exact, the squared deviations tc_ffn_dw_fwd leaves, is held by the bound derived in
test_ffn_dw_fwd_statistics.

Alignment: a kernel is only called with operands aligned to its own access width.  The fp32 strip instantiations are reachable only through
a base that is not 16-byte aligned, which their own float4 accesses would not survive: they have no aligned caller and no case here."""
import ctypes as C

import pytest
import torch

import dw_ref as R

pytestmark = pytest.mark.gpu

from transception_amd._lib import TC_BF16, TC_F16, TC_F32, TcDwFold, TcDwSeg, TcError, lib  # noqa: E402

DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
HALF = [torch.bfloat16, torch.float16]
TC = {torch.float32: TC_F32, torch.bfloat16: TC_BF16, torch.float16: TC_F16}
ids = lambda d: str(d).split(".")[-1]  # noqa: E731
EACH_DTYPE = pytest.mark.parametrize("dtype", DTYPES, ids=ids)
EACH_HALF = pytest.mark.parametrize("dtype", HALF, ids=ids)
REJECT = dict(match="status -1")                                           # TC_ERR_ARG
WS_BYTES = 8 << 20
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]


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


def ready(p):
    """The premise of a case, asserted once per Prob: grids and sum|term| / quantum < 2^24 for its three reductions."""
    if not p.__dict__.get("_ready"):
        assert p.premise()
        p._ready = True
    return p


_HOST = {"x": lambda p: p.x, "dy": lambda p: p.dy, "w": lambda p: p.w, "b": lambda p: p.b}


def D(p, name):
    """Device copy of an input of p (uploaded once; nothing may write to it: `untouched`)."""
    d = p.__dict__.setdefault("_dev", {})
    if name not in d:
        d[name] = up(_HOST[name](p).flat)
    return d[name]


def A(p, name):
    return addr(D(p, name), getattr(_HOST[name](p), "lead", 0))


def untouched(p):
    for name, t in p.__dict__.get("_dev", {}).items():
        same_bits(t, _HOST[name](p).flat, f"{p.tag}: {name} is only read")


_ws = None


def ws():
    """The TcGemm.ws-style workspace: 16 KiB of arrival counters, zero before and after every launch, then room for the walkers' sums."""
    global _ws
    if _ws is None:
        _ws = torch.zeros(WS_BYTES, dtype=torch.uint8, device=DEV)
    return _ws


def plan(p):
    site = TcDwFold()
    nf = int(lib().tc_dwconv_bwd_plan(p.B, p.H, p.W, p.C, p.k, p.groups, TC[p.dtype], C.byref(site)))
    return nf, site


def ws_args(p, form):
    """(ws, ws_bytes, check()) of the four workspace forms of a weight-gradient launch."""
    if form == "null":                                                     # walk_ws: no workspace -> plain atomics
        return None, 0, lambda: None
    w, nf = ws(), plan(p)[0]
    if form == "ws":                                                       # usable -> parked sums, arrival counters, two-level fold
        assert nf == 0 or 16384 + 4 * nf <= WS_BYTES

        def zero():
            assert int(w[:16384].count_nonzero()) == 0, f"{p.tag}: the arrival counters must be zero again"
        return addr(w), WS_BYTES, zero
    before = w.clone()
    keep = lambda: same_bits(w, before.cpu(), f"{p.tag}: an unusable workspace is not written")  # noqa: E731
    if form == "small":                                                    # one float short of counters + sums: legal, unusable -> atomics
        assert nf > 0
        return addr(w), 16384 + 4 * nf - 4, keep
    assert form == "unaligned"                                             # large enough, 4 bytes off the 16-byte grid -> atomics
    return addr(w, 4), WS_BYTES - 4, keep


def dims(p):
    return p.B, p.H, p.W, p.C, p.k


# ---------------------------------------------------------------------------------------------------------------- one entry, one call, whole buffers
def run_fwd(p, bias, add):
    y0 = p.y0()
    yd = up(y0.flat)
    lib().tc_dwconv_fwd(A(p, "x"), p.ld["x"], A(p, "w"), A(p, "b") if bias else None, addr(yd, y0.lead), p.ld["y"], *dims(p), p.stride, add,
                        p.groups, p.wstride, TC[p.dtype], stream())
    sync()
    exact(yd, y0.expect(p.ref_fwd(bias, add)), f"{p.tag}: y bias={bias} add={add}")


def run_bwd_input(p, add, acc):
    d0 = p.dx0(acc)
    dd = up(d0.flat)
    lib().tc_dwconv_bwd_input(A(p, "dy"), p.ld["dy"], A(p, "w"), addr(dd, d0.lead), p.ld["dx"], *dims(p), p.stride, add, acc, p.groups, p.wstride,
                              TC[p.dtype], stream())
    sync()
    exact(dd, d0.expect(p.ref_bwd_input(add), acc), f"{p.tag}: dx add={add} acc={acc}")


def want_grads(p, dw0, db0):
    dw, db = p.ref_bwd_weight()
    return dw0.expect_add(dw.reshape(p.groups, -1)), db0.expect_add(db)


def run_bwd_weight(p, form, with_db=True):
    dw0, db0 = p.dw0(), p.db0()
    dwd, dbd = up(dw0.flat), up(db0.flat)
    wsp, wsb, check = ws_args(p, form)
    lib().tc_dwconv_bwd_weight(A(p, "dy"), p.ld["dy"], A(p, "x"), p.ld["x"], addr(dwd), addr(dbd) if with_db else None, *dims(p), p.stride, p.groups,
                               p.wstride, wsp, wsb, TC[p.dtype], stream())
    sync()
    wdw, wdb = want_grads(p, dw0, db0)
    exact(dwd, wdw, f"{p.tag}: dw ws={form}")
    exact(dbd, wdb if with_db else db0.flat.double(), f"{p.tag}: db ws={form}")
    check()


def fold_one(site, part, dwd, dbd, wstride, off=0):
    site.part, site.dw, site.db, site.dgamma, site.dbeta, site.wstride = addr(part, off), addr(dwd), addr(dbd) if dbd is not None else None, None, None, wstride
    return site


def run_bwd(p, add, acc, form):
    """tc_dwconv_bwd: both gradients; form "defer": the sums parked in a buffer of the plan's size, dw / db untouched until tc_dw_fold."""
    d0, dw0, db0 = p.dx0(acc), p.dw0(), p.db0()
    dd, dwd, dbd = up(d0.flat), up(dw0.flat), up(db0.flat)
    if form == "defer":
        nf, site = plan(p)
        assert nf > 0 and nf == site.chunks * p.groups * site.gx * site.nt * site.ch
        part = torch.full((nf + 2,), R.NAN, dtype=torch.float32, device=DEV)
        wsp, wsb, check = addr(part), -4 * nf, lambda: None
    else:
        wsp, wsb, check = ws_args(p, form)
    lib().tc_dwconv_bwd(A(p, "dy"), p.ld["dy"], A(p, "x"), p.ld["x"], A(p, "w"), addr(dd, d0.lead), p.ld["dx"], addr(dwd), addr(dbd), *dims(p), add, acc,
                        p.groups, p.wstride, wsp, wsb, TC[p.dtype], stream())
    sync()
    exact(dd, d0.expect(p.ref_bwd_input(add), acc), f"{p.tag}: dx of bwd add={add} acc={acc} ws={form}")
    wdw, wdb = want_grads(p, dw0, db0)
    if form == "defer":
        same_bits(dwd, dw0.flat, f"{p.tag}: dw waits for the fold")
        same_bits(dbd, db0.flat, f"{p.tag}: db waits for the fold")
        assert bool(part[nf:].isnan().all()) and not bool(part[:nf].isnan().any()), f"{p.tag}: the walkers fill exactly the planned floats"
        lib().tc_dw_fold(C.byref(fold_one(site, part, dwd, dbd, p.wstride)), 1, stream())
        sync()
    exact(dwd, wdw, f"{p.tag}: dw of bwd ws={form}")
    exact(dbd, wdb, f"{p.tag}: db of bwd ws={form}")
    check()


# ---------------------------------------------------------------------------------------------------------------- tile kernels
@EACH_DTYPE
@pytest.mark.parametrize("cg", R.CGS)
@pytest.mark.parametrize("k", R.KS)
def test_tile_kernels_on_map_edges(k, cg, dtype):
    """dw_tile_kernel<k, cg, 0 / 1>, dw_tile_wgrad_kernel<k, cg> and dw_tile_bwd_kernel<k, cg>: C % VEC == 0, every ld % VEC == 0, 16-byte bases
    (dw_tile_ok), C = cg vectors so that dw_pick_cg returns cg.  Maps: R.edge_maps -- a first, an interior and a last partial tile in both
    directions, B = 1 / 3, groups 1 / 2.  Forward with and without bias and + x; input gradient with and without + dy and accumulate; weight
    gradient through atomics (ws NULL), a usable workspace and the two unusable ones; both gradients in one launch, tail-folded and deferred."""
    forms = ["null", "ws", "small", "unaligned", "ws", "null"]
    for i, m in enumerate(R.edge_maps(cg)):
        p = ready(R.tile_prob(dtype, k, cg, m))
        assert R.tile_geom(p.B, p.H, p.W, p.C, R.vec_of(dtype))[0] == cg
        for bias, add in FLAGS:
            run_fwd(p, bias, add)
        for add, acc in FLAGS:
            run_bwd_input(p, add, acc)
        run_bwd_weight(p, forms[i], with_db=i != 3)
        run_bwd(p, *FLAGS[i % 4], "defer" if i % 2 else "ws")
        untouched(p)


@EACH_DTYPE
@pytest.mark.parametrize("ci", range(5))
def test_tile_kernels_partial_and_several_chunks(ci, dtype):
    """R.chunk_cs: a last chunk that is partial for each of cg = 2 / 4 / 8 (fp32 C = 20 / 12 / 28, 16-bit 40 / 24 / 56: the lanes past C are
    zeroed on the way to LDS and never stored) and three whole chunks (fp32 96 / 48), on a 2 x 9 x 19 map, k = 3, 5, 7."""
    Cc, cg, chunks, partial = R.chunk_cs(R.vec_of(dtype))[ci]
    for k in R.KS:
        p = ready(R.chunk_prob(dtype, Cc, k))
        assert R.tile_geom(p.B, p.H, p.W, Cc, R.vec_of(dtype))[:3] == (cg, cg * R.vec_of(dtype), chunks)
        run_fwd(p, 1, 1)
        run_fwd(p, 0, 0)
        run_bwd_input(p, 1, 1)
        run_bwd_input(p, 0, 0)
        run_bwd_weight(p, "ws")
        run_bwd_weight(p, "null", with_db=False)
        run_bwd(p, 1, 0, "defer")
        untouched(p)


# ---------------------------------------------------------------------------------------------------------------- strip kernels (16-bit)
@EACH_HALF
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("why", list(R.STRIP_WHY))
def test_strip_kernels(why, k, dtype):
    """dw_strip_kernel<k, CPT, 0 / 1 / 2> (CPT = 4 channels per thread for k = 3, 2 for k = 5, 7): the dispatcher leaves the tile kernels when
    dw_tile_ok fails -- C % 8 == 4, an ld % 8 == 4, or a base that is 8-byte but not 16-byte aligned (R.STRIP_WHY; every operand keeps the 8-byte
    alignment of the CPT = 4 accesses).  Maps: R.STRIP_MAPS -- rows split into two W-segments that do not divide W, one segment, W < k, groups 2.
    tc_dwconv_bwd falls back to the two single entries (ws >= 0).  With only the WRITTEN operand off the grid the weight gradient, which reads
    x and dy alone, stays on the tile kernel."""
    for i, m in enumerate(R.STRIP_MAPS[k]):
        p = ready(R.strip_prob(dtype, why, k, m))
        vec = R.vec_of(dtype)
        off = lambda *names: any(p.ld[n] % vec or p.lead.get(n, 0) % vec for n in names) or p.C % vec != 0  # noqa: E731
        assert off("x", "y") and off("dy", "dx") and (off("x", "dy") or why == "out base%16==8")
        for bias, add in FLAGS:
            run_fwd(p, bias, add)
        for add, acc in FLAGS:
            run_bwd_input(p, add, acc)
        run_bwd_weight(p, "ws" if i % 2 else "null", with_db=i != 2)
        run_bwd(p, *FLAGS[i % 4], "ws")
        untouched(p)


# ---------------------------------------------------------------------------------------------------------------- stride 2
@EACH_DTYPE
@pytest.mark.parametrize("k", R.KS)
@pytest.mark.parametrize("Cc", R.STRIDE2_CS)
def test_stride2_kernels(Cc, k, dtype):
    """stride == 2: dw_kernel<k, false, 2> (forward), dw_kernel<k, true, 2> (input gradient, with and without accumulate), dw_wgrad3_kernel
    (k = 3, both ld % 4 == 0 -- which the entry now demands) and dw_wgrad_kernel<5 / 7>.  Odd and even H and W, H != W, maps smaller than the
    filter; C = 8 (one partial 64-channel block) and 68 (two blocks)."""
    for m in R.STRIDE2_MAPS:
        p = ready(R.stride2_prob(dtype, Cc, k, m))
        assert (p.Ho, p.Wo) == ((p.H + 1) // 2, (p.W + 1) // 2)
        run_fwd(p, 0, 0)
        run_fwd(p, 1, 0)
        run_bwd_input(p, 0, 0)
        run_bwd_input(p, 0, 1)
        run_bwd_weight(p, "null")
        run_bwd_weight(p, "ws", with_db=False)                                # (the workspace is not used off the tile kernels)
        untouched(p)


# ---------------------------------------------------------------------------------------------------------------- walker tails
@EACH_DTYPE
@pytest.mark.parametrize("name", ["gx<ntiles", "gx%4!=0", "gx==3", "gx==1"])
def test_weight_gradient_walker_tails(name, dtype):
    """dw_walker_tail's three ways out, on the same tile launch in four forms: ws NULL (atomics), a usable workspace (write-through parking,
    one arrival counter per DW_FOLD = 4 walkers, the last arriver folds), a legal but unusable workspace (one float short; 4 bytes off: atomics),
    and tc_dwconv_bwd with ws_bytes < 0 followed by tc_dw_fold.  dw / db are bit-identical to the reference each time and the counters zero again.
    The premise of each case is read from tc_dwconv_bwd_plan and asserted: gx < ntiles (a walker visits several tiles, unevenly; the fold
    kernel's unrolled 32-walker loop and its remainder both run: gx = 85), gx % 4 != 0 with gx > 4 (a short last arrival group), gx = 3 (one
    short group; tc_dw_fold with gx < 4) and gx = 1 (nothing parked)."""
    p = ready(R.walker_prob(dtype, name))
    nf, site = plan(p)
    ntiles = R.tile_geom(p.B, p.H, p.W, p.C, R.vec_of(dtype))[4]
    assert nf > 0 and R.walker_premise(name, site.gx, ntiles), (name, site.gx, ntiles)
    assert site.chunks * p.groups * ((site.gx + 3) // 4) <= 4096 and 16384 + 4 * nf <= WS_BYTES      # the workspace form is usable
    for form in ("null", "ws", "small", "unaligned"):
        run_bwd_weight(p, form)
    run_bwd(p, 1, 0, "ws")
    run_bwd(p, 0, 1, "defer")
    untouched(p)


# ---------------------------------------------------------------------------------------------------------------- tc_dw_fold on hand-filled sums
def _site(Cc, k, groups, ch, gx, nt, wstride):
    s = TcDwFold()
    s.C, s.k, s.groups, s.ch, s.chunks, s.gx, s.nt, s.wstride = Cc, k, groups, ch, -(-Cc // ch), gx, nt, wstride
    return s


def test_dw_fold_sites():
    """tc_dw_fold alone, several sites in one call: different k, C, chunk widths and groups; gx = 70 (wsplit 3: the unrolled 32-walker loop and
    its remainder) and gx = 1, 3 (< 4); two sites that add into the same dw / db (a convolution used twice); a site with db = NULL; groups = 3
    with wstride larger than the parameter block (the words between the groups keep the sentinel); nt = k k + 3 with dgamma / dbeta (the
    tc_ffn_mid_bwd routing); a partial last chunk whose spare channels hold NaN.  Sums are quarters: every fp32 sum is exact."""
    L = lib()
    #        C   k  groups ch  gx  nt       wstride  target  db
    spec = [(20, 3, 1, 8, 70, 10, 0, "a", True),
            (20, 3, 1, 8, 3, 10, 0, "a", True),                               # the same dw / db as the first site
            (12, 5, 3, 16, 1, 26, 12 * 25 + 7, "b", False),                   # db = NULL
            (64, 7, 2, 32, 33, 50, 64 * 49 + 4, "c", True),
            (24, 3, 2, 16, 37, 12, 24 * 9 + 8, "d", True)]                    # nt = 12: dgamma / dbeta
    tgt, want, sites, keep = {}, {}, [], []
    for i, (Cc, k, G, ch, gx, nt, wst, name, with_db) in enumerate(spec):
        kk, chunks = k * k, -(-Cc // ch)
        part = R.quarters(f"fold/{i}", (G * chunks, gx, nt, ch))
        part.view(G, chunks, gx, nt, ch)[:, -1, :, :, Cc - (chunks - 1) * ch:] = R.NAN      # past C: read, added, never routed
        assert float(part.nan_to_num().abs().sum(dim=1).max()) / 0.25 < 2.0 ** 24
        if name not in tgt:
            names = ("dw", "db") + (("dgamma", "dbeta") if nt == kk + 3 else ())
            tgt[name] = {n: R.Params(f"fold/{name}/{n}", Cc * kk if n == "dw" else Cc, G, wst, torch.float32, R.halves, R.SENT) for n in names}
            want[name] = {n: t.flat.double().clone() for n, t in tgt[name].items()}
            for t in tgt[name].values():
                t.dev = up(t.flat)
        sums = R.fold(part, Cc, kk, ch, chunks, gx, nt, G)                     # [G, nt, C]
        t = tgt[name]
        for g in range(G):
            want[name]["dw"][g * wst:g * wst + Cc * kk] += sums[g, :kk].t().reshape(-1)          # dw is [C][k k]
            for n, row in (("db", kk), ("dgamma", kk + 1), ("dbeta", kk + 2)):
                if n in t and (n != "db" or with_db):
                    want[name][n][g * wst:g * wst + Cc] += sums[g, row]
        s = _site(Cc, k, G, ch, gx, nt, wst)
        pd = up(part.reshape(-1))
        keep.append((pd, part.reshape(-1)))
        s.part, s.dw, s.db = addr(pd), addr(t["dw"].dev), addr(t["db"].dev) if with_db else None
        s.dgamma, s.dbeta = (addr(t["dgamma"].dev), addr(t["dbeta"].dev)) if "dgamma" in t else (None, None)
        sites.append(s)
    L.tc_dw_fold((TcDwFold * len(sites))(*sites), len(sites), stream())
    sync()
    for name in tgt:
        for n, t in tgt[name].items():
            exact(t.dev, want[name][n], f"fold {name}.{n}")
    for pd, host in keep:
        same_bits(pd, host, "the parked sums are only read")
    # rejected before the launch: n = 0, n = 49, and each inconsistent geometry
    arr49 = (TcDwFold * 49)(*([sites[0]] * 49))
    with pytest.raises(TcError, **REJECT):
        L.tc_dw_fold(arr49, 0, stream())
    with pytest.raises(TcError, **REJECT):
        L.tc_dw_fold(arr49, 49, stream())
    for field, bad in (("chunks", 2), ("nt", 11), ("k", 4), ("gx", 0), ("ch", 0), ("groups", 0), ("C", 0), ("part", None), ("dw", None)):
        s = TcDwFold()
        C.memmove(C.byref(s), C.byref(sites[0]), C.sizeof(TcDwFold))
        setattr(s, field, bad)
        with pytest.raises(TcError, **REJECT):
            L.tc_dw_fold(C.byref(s), 1, stream())
    sync()
    for name in tgt:
        for n, t in tgt[name].items():
            exact(t.dev, want[name][n], f"fold {name}.{n} after the rejected calls")


# ---------------------------------------------------------------------------------------------------------------- tc_dwconv_multi
class Placed:
    """Where the segments' operand `name` lives: each Prob's own buffer, or column slices of one wide map (ld = all channels + pad vectors)."""

    def __init__(self, probs, name, wide, pad, out=False, acc=False):
        dtype, vec = probs[0].dtype, R.vec_of(probs[0].dtype)
        rows = [p.rout if name in ("y", "dy") else p.rin for p in probs]
        if not wide:
            own = {"x": lambda p: p.x, "dy": lambda p: p.dy, "y": lambda p: p.y0(acc), "dx": lambda p: p.dx0(acc)}[name]
            self.maps = [own(p) for p in probs]
            self.bufs = [m.flat for m in self.maps]
            self.idx = list(range(len(probs)))
        else:
            assert len(set(rows)) == 1
            tot = sum(p.C for p in probs)
            big = (R.out_map if out else R.in_map)(f"{probs[0].tag}/wide/{name}", rows[0], tot, tot + pad * vec, dtype, **({"acc": acc} if out else {}))
            offs = [sum(q.C for q in probs[:i]) for i in range(len(probs))]
            self.maps = [big.cols(o, p.C) for o, p in zip(offs, probs)]
            if not out:
                for m, p in zip(self.maps, probs):
                    m.logical().copy_((p.x if name == "x" else p.dy).logical())
            self.bufs, self.idx = [big.flat], [0] * len(probs)
        self.dev = [up(b) for b in self.bufs]

    def ptr(self, i):
        return addr(self.dev[self.idx[i]], self.maps[i].lead)

    def ld(self, i):
        return self.maps[i].ld

    def check(self, vals, acc, what):
        """Every buffer, whole, against the float64 expectation: vals[i] written to (added into) segment i's place; None: an input, unchanged."""
        if vals is None:
            for d, b in zip(self.dev, self.bufs):
                same_bits(d, b, what + " is only read")
            return
        want = [b.double().clone() for b in self.bufs]
        for i, v in enumerate(vals):
            self.maps[i].write(want[self.idx[i]], v, acc)
        for d, w in zip(self.dev, want):
            exact(d, w, what)


def _multi(probs, wide, mode, add, acc, ws_form, expect_error=False):
    L, n, G, tc = lib(), len(probs), probs[0].groups, TC[probs[0].dtype]
    wst = R.MULTI_WSTRIDE
    assert all(p.groups == G and p.wstride == wst for p in probs)
    for p in probs:
        ready(p)
    x, dy = Placed(probs, "x", wide, 1), Placed(probs, "dy", wide, 3)
    y = Placed(probs, "y", wide, 2, True) if mode == 0 else None
    dx = Placed(probs, "dx", wide, 4, True, acc) if mode in (1, 3) else None
    dw0, db0 = [p.dw0() for p in probs], [p.db0() for p in probs]
    dwd, dbd = [up(t.flat) for t in dw0], [up(t.flat) for t in db0]
    segs = (TcDwSeg * n)()
    for i, p in enumerate(probs):
        g = (p.C, p.k)
        hw = (p.B, p.H, p.W, None)
        if mode == 0:
            segs[i] = TcDwSeg(x.ptr(i), A(p, "w"), A(p, "b") if i != 1 else None, y.ptr(i), None, None, None, *g, x.ld(i), y.ld(i), 0, *hw)
        elif mode == 1:
            segs[i] = TcDwSeg(dy.ptr(i), A(p, "w"), None, dx.ptr(i), None, None, None, *g, dy.ld(i), dx.ld(i), 0, *hw)
        elif mode == 2:
            segs[i] = TcDwSeg(x.ptr(i), None, None, None, dy.ptr(i), addr(dwd[i]), addr(dbd[i]) if i != 1 else None, *g, x.ld(i), 0, dy.ld(i), *hw)
        else:
            segs[i] = TcDwSeg(x.ptr(i), A(p, "w"), None, dx.ptr(i), dy.ptr(i), addr(dwd[i]), addr(dbd[i]), *g, x.ld(i), dx.ld(i), dy.ld(i), *hw)
    part = None
    if ws_form == "defer":
        sites, offs = (TcDwFold * n)(), (C.c_longlong * n)()
        nf = int(L.tc_dwconv_multi_plan(segs, n, G, tc, sites, offs))
        assert nf > 0
        part = torch.full((nf + 2,), R.NAN, dtype=torch.float32, device=DEV)
        wsp, wsb, zero = addr(part), -4 * nf, lambda: None
    elif ws_form == "ws":
        wsp, wsb = addr(ws()), WS_BYTES
        zero = lambda: int(ws()[:16384].count_nonzero()) == 0 or pytest.fail("the arrival counters must be zero again")  # noqa: E731
    else:
        wsp, wsb, zero = None, 0, lambda: None
    call = lambda: L.tc_dwconv_multi(segs, n, mode, add, acc, G, wst, wsp, wsb, tc, stream())  # noqa: E731
    what = f"{probs[0].tag} mode {mode} add={add} acc={acc} ws={ws_form}"
    if expect_error:
        with pytest.raises(TcError, **REJECT):
            call()
        sync()
        dx.check([torch.zeros(p.rin, p.C, dtype=torch.float64) for p in probs], True, what + ": dx untouched")
        for i in range(n):
            same_bits(dwd[i], dw0[i].flat, what + ": dw untouched")
            same_bits(dbd[i], db0[i].flat, what + ": db untouched")
        assert bool(part.isnan().all()), what + ": the deferred buffer untouched"
        return
    call()
    sync()
    if mode == 0:
        y.check([p.ref_fwd(i != 1, add) for i, p in enumerate(probs)], False, what + ": y")
    if mode in (1, 3):
        dx.check([p.ref_bwd_input(add) for p in probs], acc, what + ": dx")
    if mode >= 2:
        if part is not None:
            for i in range(n):
                same_bits(dwd[i], dw0[i].flat, what + ": dw waits for the fold")
            assert bool(part[nf:].isnan().all()) and not bool(part[:nf].isnan().any()), what + ": the walkers fill exactly the planned floats"
            arr = (TcDwFold * n)(*[fold_one(sites[i], part, dwd[i], dbd[i], wst, int(offs[i])) for i in range(n)])
            L.tc_dw_fold(arr, n, stream())
            sync()
        for i, p in enumerate(probs):
            wdw, wdb = want_grads(p, dw0[i], db0[i])
            exact(dwd[i], wdw, what + f": dw[{i}]")
            exact(dbd[i], wdb if (mode == 3 or i != 1) else db0[i].flat.double(), what + f": db[{i}]")
        zero()
    x.check(None, False, what + ": x")
    dy.check(None, False, what + ": dy")
    for p in probs:
        untouched(p)


@EACH_DTYPE
@pytest.mark.parametrize("case", ["crpe g1", "crpe g3", "maps"])
def test_multi_one_launch(case, dtype):
    """tc_dwconv_multi with every segment tile-eligible -> launch_multi: dw_multi_kernel<0 / 1>, dw_multi_wgrad_kernel, dw_multi_bwd_kernel.
    crpe: k = 3 / 5 / 7 on three column slices of ONE wide map (different C, one ld), groups 1 and 3; maps: four segments on maps of their own.
    Modes 0 to 3; a NULL bias (mode 0) and a NULL db (mode 2) on segment 1; mode 2 / 3 with ws NULL and a usable workspace; mode 3 with the
    deferred buffer of tc_dwconv_multi_plan, then ONE tc_dw_fold over the segments' sites."""
    probs, wide = R.multi_cases(dtype)[case]
    vec = R.vec_of(dtype)
    assert all(p.C % vec == 0 for p in probs)
    _multi(probs, wide, 0, 0, 0, None)
    _multi(probs, wide, 0, 1, 0, None)
    _multi(probs, wide, 1, 0, 1, None)
    _multi(probs, wide, 1, 1, 0, None)
    _multi(probs, wide, 2, 0, 0, None)
    _multi(probs, wide, 2, 0, 0, "ws")
    _multi(probs, wide, 3, 1, 1, "ws")
    _multi(probs, wide, 3, 0, 0, None)
    _multi(probs, wide, 3, 1, 0, "defer")


@EACH_HALF
@pytest.mark.parametrize("case", ["fallback", "fallback g3"])
def test_multi_per_segment_fallback(case, dtype):
    """One segment with ld % 8 == 4 (x and dy) makes the launch ineligible: modes 0, 1, 2 go segment by segment through tc_dwconv_fwd /
    tc_dwconv_bwd_input / tc_dwconv_bwd_weight, mode 3 through tc_dwconv_bwd (the eligible segment on the tile kernels, the other on the strip
    kernels).  Deferred sums are refused BEFORE anything is launched (dx, dw, db and the buffer untouched): through the single entries the
    eligible segment would have parked its sums in the single launch's layout at offset 0, not at the plan's offs[i], and written its dx."""
    probs, wide = R.multi_cases(dtype)[case]
    assert probs[1].ld["x"] % 8 == 4 and probs[1].ld["dy"] % 8 == 4 and probs[0].ld["x"] % 8 == 0
    for mode, add, acc, form in ((0, 1, 0, None), (1, 1, 1, None), (2, 0, 0, "ws"), (2, 0, 0, None), (3, 1, 1, "ws"), (3, 0, 0, None)):
        _multi(probs, wide, mode, add, acc, form)
    _multi(probs, wide, 3, 1, 0, "defer", expect_error=True)


# ---------------------------------------------------------------------------------------------------------------- tc_ffn_dw_fwd
@EACH_DTYPE
def test_ffn_dw_fwd_statistics(dtype):
    """tc_ffn_dw_fwd: y = dw3x3(x) + bias + x exactly, and stat = (sum, squared deviations from the chunk mean) per pixel and chunk of
    CH = tc_ffn_chunk channels, computed from the UNROUNDED fp32 result (dw_tile_body's acc, before tc_pack16), so the reference is
    R.chunk_stats of the float64 result, not of the stored y.

    The sum is exact (multiples of 1/8, far below 2^24 of them).  The squared deviations are not; the bound follows the kernel:
      mu = sum * (1 / CH): exact, CH is a power of two (asserted);
      d = acc - mu: exact -- both are multiples of 1 / (8 CH) and |d| <= 2 max|acc| stays below 2^24 such quanta (asserted: the reference's
          deviations are float32 values);
      d * d rounds once (or not at all where the compiler contracts it into the add), a thread adds its VEC squares in sequence and
      tc_group_sum adds the CG lanes in log2(CG) steps: a term passes at most 1 + (VEC - 1) + log2(CG) roundings of relative size 2^-24, all
      terms are non-negative, so |got - m2| <= ((1 + 2^-24)^(VEC + log2 CG) - 1) m2 <= CH 2^-24 m2, since VEC + log2 CG <= VEC CG = CH and
      CH 2^-24 << 1.  The bound is c CH 2^-24 m2 with c = 1.
    stat = NULL leaves y alone; C % CH != 0 with stat is TC_ERR_ARG before the launch."""
    L, tc, vec = lib(), TC[dtype], R.vec_of(dtype)
    for Cc, G in R.ffn_cases(vec):
        p = ready(R.ffn_prob(dtype, Cc, G))
        ch = int(L.tc_ffn_chunk(Cc, tc))
        assert Cc % ch == 0 and ch & (ch - 1) == 0
        ref = p.ref_fwd(True, True)
        want = R.chunk_stats(ref, ch)                                         # [N, H, W, nch, 2]
        v = ref.reshape(*ref.shape[:-1], Cc // ch, ch)
        assert R.is_f32_value(want[..., 0]) and R.is_f32_value(v - want[..., 0:1] / ch)
        n = want.numel()
        for with_stat in (True, False):
            y0 = p.y0()
            yd = up(y0.flat)
            st = torch.full((n + 2,), R.SENT, dtype=torch.float32, device=DEV)
            L.tc_ffn_dw_fwd(A(p, "x"), p.ld["x"], A(p, "w"), A(p, "b"), addr(yd), p.ld["y"], addr(st) if with_stat else None, p.B, p.H, p.W, Cc, G,
                            p.wstride, tc, stream())
            sync()
            exact(yd, y0.expect(ref), f"{p.tag}: y stat={with_stat}")
            got = st.cpu().double()
            assert bool((got[n:] == R.SENT).all())
            if not with_stat:
                assert bool((got == R.SENT).all())
                continue
            got = got[:n].reshape(want.shape)
            assert torch.equal(got[..., 0], want[..., 0]), f"{p.tag}: chunk sums"
            err, bound = (got[..., 1] - want[..., 1]).abs(), ch * 2.0 ** -24 * want[..., 1]
            print(f"\n[ffn_dw] {p.tag}: largest error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}, largest error {float(err.max()):.3e}")
            assert bool((err <= bound).all()), (p.tag, float(err.max()))
            # the same body through tc_dwconv_multi (mode 0, one k = 3 segment with stat): the same y and the same statistics, bit for bit
            yd2, st2 = up(y0.flat), torch.full((n + 2,), R.SENT, dtype=torch.float32, device=DEV)
            seg = (TcDwSeg * 1)(TcDwSeg(A(p, "x"), A(p, "w"), A(p, "b"), addr(yd2), None, None, None, Cc, 3, p.ld["x"], p.ld["y"], 0, p.B, p.H, p.W,
                                        addr(st2)))
            L.tc_dwconv_multi(seg, 1, 0, 1, 0, G, p.wstride, None, 0, tc, stream())
            sync()
            exact(yd2, y0.expect(ref), f"{p.tag}: y of the multi launch with stat")
            same_bits(st2, st.cpu(), f"{p.tag}: stat of the multi launch")
        untouched(p)
    p = ready(R.chunk_prob(dtype, R.chunk_cs(vec)[0][0], 3))                    # fp32 C = 20, 16-bit C = 40: chunks of 2 vectors, the last partial
    assert p.C % int(L.tc_ffn_chunk(p.C, tc)) != 0
    y0 = p.y0()
    yd, st = up(y0.flat), torch.full((4096,), R.SENT, dtype=torch.float32, device=DEV)
    with pytest.raises(TcError, **REJECT):
        L.tc_ffn_dw_fwd(A(p, "x"), p.ld["x"], A(p, "w"), A(p, "b"), addr(yd), p.ld["y"], addr(st), p.B, p.H, p.W, p.C, 1, p.wstride, tc, stream())
    sync()
    same_bits(yd, y0.flat, "y after the rejected call")
    assert bool((st == R.SENT).all())
    L.tc_ffn_dw_fwd(A(p, "x"), p.ld["x"], A(p, "w"), None, addr(yd), p.ld["y"], None, p.B, p.H, p.W, p.C, 1, p.wstride, tc, stream())       # fine without stat
    sync()
    exact(yd, y0.expect(p.ref_fwd(False, True)), f"{p.tag}: y, partial chunk, no bias, no stat")


# ---------------------------------------------------------------------------------------------------------------- rejections
@EACH_DTYPE
def test_rejections_leave_the_outputs_alone(dtype):
    """Every TC_ERR_ARG the entries state is host-side, before any launch: after all of them y, dx, dw, db and the deferred buffer still hold what
    they held.  C % 4 != 0, k not in {3, 5, 7}, stride not in {1, 2}, + x with stride 2, groups > 1 with stride 2, an ld % 4 != 0 (each ld of
    each entry -- tc_dwconv_bwd_weight's two and tc_dwconv_bwd's ldx were not checked before), a deferred buffer on operands that do not allow the
    tile kernel, one smaller than the plan's or unaligned, and tc_dwconv_multi's own."""
    L, tc, s = lib(), TC[dtype], stream()
    p = ready(R.tile_prob(dtype, 3, 2, R.edge_maps(2)[1]))                     # (1, 2, 5), groups 2, cg 2
    B, H, W, Cc, k = dims(p)
    G, wst, ld = p.groups, p.wstride, p.ld
    y0, d0, dw0, db0 = p.y0(), p.dx0(), p.dw0(), p.db0()
    yd, dd, dwd, dbd = up(y0.flat), up(d0.flat), up(dw0.flat), up(db0.flat)
    nf, _ = plan(p)
    part = torch.full((nf + 4,), R.SENT, dtype=torch.float32, device=DEV)
    x, w, b, dy, yp, dxp, dw, db = A(p, "x"), A(p, "w"), A(p, "b"), A(p, "dy"), addr(yd), addr(dd), addr(dwd), addr(dbd)

    def fwd(Cc=Cc, k=k, stride=1, add=0, G=G, ldx=ld["x"], ldy=ld["y"]):
        L.tc_dwconv_fwd(x, ldx, w, b, yp, ldy, B, H, W, Cc, k, stride, add, G, wst, tc, s)

    def bwi(Cc=Cc, k=k, stride=1, add=0, G=G, lddy=ld["dy"], lddx=ld["dx"]):
        L.tc_dwconv_bwd_input(dy, lddy, w, dxp, lddx, B, H, W, Cc, k, stride, add, 0, G, wst, tc, s)

    def bww(Cc=Cc, k=k, stride=1, G=G, lddy=ld["dy"], ldx=ld["x"]):
        L.tc_dwconv_bwd_weight(dy, lddy, x, ldx, dw, db, B, H, W, Cc, k, stride, G, wst, None, 0, tc, s)

    def bwd(Cc=Cc, k=k, add=0, G=G, lddy=ld["dy"], ldx=ld["x"], lddx=ld["dx"], wsp=None, wsb=0, xp=x):
        L.tc_dwconv_bwd(dy, lddy, xp, ldx, w, dxp, lddx, dw, db, B, H, W, Cc, k, add, 0, G, wst, wsp, wsb, tc, s)

    bad = [lambda: fwd(Cc=Cc + 2), lambda: fwd(k=4), lambda: fwd(k=9), lambda: fwd(stride=3), lambda: fwd(stride=0), lambda: fwd(stride=2, add=1, G=1),
           lambda: fwd(stride=2), lambda: fwd(G=0), lambda: fwd(ldx=ld["x"] + 2), lambda: fwd(ldy=ld["y"] + 1),
           lambda: bwi(Cc=Cc + 2), lambda: bwi(k=4), lambda: bwi(stride=3), lambda: bwi(stride=2, add=1, G=1), lambda: bwi(stride=2),
           lambda: bwi(lddy=ld["dy"] + 2), lambda: bwi(lddx=ld["dx"] + 3),
           lambda: bww(Cc=Cc + 2), lambda: bww(k=6), lambda: bww(stride=3), lambda: bww(stride=2), lambda: bww(lddy=ld["dy"] + 2), lambda: bww(ldx=ld["x"] + 2),
           lambda: bww(stride=2, G=1, lddy=ld["dy"] + 2), lambda: bww(stride=2, G=1, ldx=ld["x"] + 1),
           lambda: bwd(Cc=Cc + 2), lambda: bwd(k=4), lambda: bwd(lddy=ld["dy"] + 2), lambda: bwd(lddx=ld["dx"] + 2), lambda: bwd(ldx=ld["x"] + 2),
           lambda: bwd(G=0),
           lambda: bwd(wsp=addr(part), wsb=-4 * (nf - 1)),                    # a deferred buffer smaller than the plan's
           lambda: bwd(wsp=addr(part, 1), wsb=-4 * nf),                       # ... or off the 16-byte grid
           lambda: bwd(wsp=addr(part), wsb=-4 * nf, xp=x + 8)]                # ... or with an operand the tile kernels cannot take: x 8 bytes off
    if dtype != torch.float32:                                               # ... or an ld % 8 == 4 (16-bit)
        bad.append(lambda: bwd(wsp=addr(part), wsb=-4 * nf, ldx=ld["x"] + 4))
    segs = (TcDwSeg * 5)(*[TcDwSeg(x, w, b, yp, dy, dw, db, Cc, k, ld["x"], ld["y"], ld["dy"], B, H, W, None)] * 5)

    def multi(n=1, mode=0, G=G, **kw):
        sg = (TcDwSeg * 5)(*segs)
        for f, v in kw.items():
            setattr(sg[0], f, v)
        L.tc_dwconv_multi(sg, n, mode, 0, 0, G, wst, None, 0, tc, s)
    bad += [lambda: multi(n=0), lambda: multi(n=5), lambda: multi(mode=4), lambda: multi(mode=-1), lambda: multi(G=0), lambda: multi(C=Cc + 2),
            lambda: multi(k=4), lambda: multi(ldx=ld["x"] + 2), lambda: multi(ldy=ld["y"] + 2), lambda: multi(mode=2, lddy=ld["dy"] + 2),
            lambda: multi(mode=3, lddy=ld["dy"] + 2), lambda: multi(mode=2, dw=None), lambda: multi(x=None)]
    st = torch.full((64,), R.SENT, dtype=torch.float32, device=DEV)
    bad += [lambda: multi(stat=addr(st), n=1, mode=0, k=5),                   # statistics: k = 3 only
            lambda: L.tc_ffn_dw_fwd(x, ld["x"] + 2, w, b, yp, ld["y"], None, B, H, W, Cc, G, wst, tc, s),
            lambda: L.tc_ffn_dw_fwd(x + 8, ld["x"], w, b, yp, ld["y"], None, B, H, W, Cc, G, wst, tc, s)]      # no strip form: refused
    for i, f in enumerate(bad):
        with pytest.raises(TcError, **REJECT):
            f()
    sync()
    same_bits(yd, y0.flat, "y")
    same_bits(dd, d0.flat, "dx")
    same_bits(dwd, dw0.flat, "dw")
    same_bits(dbd, db0.flat, "db")
    assert bool((part == R.SENT).all()) and bool((st == R.SENT).all())
    untouched(p)
    fwd(), bwi(), bww(), bwd(wsp=addr(part), wsb=-4 * nf)                     # the same closures with nothing wrong are accepted
    sync()
    exact(yd, y0.expect(p.ref_fwd(True, False)), "the accepted forward")


# ---------------------------------------------------------------------------------------------------------------- the engine's choice
@EACH_HALF
def test_engine_keeps_ineligible_multi_off_the_deferred_form(dtype):
    """engine.Graph.dwconv_multi offers tc_dwconv_multi_plan's buffer only when every segment's x, dy and dx allow the tile kernels (dw_tile_ok
    restated, as Graph.dwconv does).  Two column slices of a 44-column map (ld % 8 == 4, the first slice 8 bytes off the 16-byte grid): the
    entry now refuses deferred sums for them, so the engine must launch the tail-folded form -- y, dx, dw and db are the reference's, exactly."""
    from transception_amd.engine import Graph, P, Var
    B, H, W, Cs, ks, off = 2, 5, 9, (16, 24), (3, 5), 4
    rows, tot = B * H * W, 4 + 16 + 24
    G = Graph(dtype, torch.device(DEV), training=True, record=True)
    x, gy = R.halves("eng/x", (rows, tot), dtype), R.halves("eng/gy", (rows, sum(Cs)), dtype)
    wts = [R.quarters(f"eng/w{i}", (c, k * k), dtype) for i, (c, k) in enumerate(zip(Cs, ks))]
    bss = [R.quarters(f"eng/b{i}", (c,), dtype) for i, c in enumerate(Cs)]
    xv = Var(up(x).contiguous(), requires_grad=True)
    out = G.new(rows, sum(Cs))
    mkP = lambda t: P(up(t).contiguous(), torch.zeros(t.shape, dtype=torch.float32, device=DEV))  # noqa: E731
    Ws, Bs = [mkP(w) for w in wts], [mkP(b) for b in bss]
    cols = [(off, off + Cs[0]), (off + Cs[0], tot)]
    xs = [xv.colslice(a, b) for a, b in cols]
    outs = [out.colslice(0, Cs[0]), out.colslice(Cs[0], sum(Cs))]
    assert xs[0].ld % 8 == 4
    G.dwconv_multi(xs, Ws, Bs, (B, H, W), list(ks), outs)
    sync()
    x4, g4 = x.reshape(B, H, W, tot), gy.reshape(B, H, W, sum(Cs))
    c0 = 0
    for i, ((a, b), k) in enumerate(zip(cols, ks)):
        exact(out.data[:, c0:c0 + Cs[i]], R.fwd(x4[..., a:b], wts[i], bss[i], k).reshape(rows, -1), f"engine y[{i}]")
        c0 += Cs[i]
    out.root.grad_t = up(gy).contiguous().view(out.rows, out.cols)
    out.root.whole_written = True
    G.backward()
    sync()
    dx, c0 = G.grad_of(xv), 0
    for i, ((a, b), k) in enumerate(zip(cols, ks)):
        gi = g4[..., c0:c0 + Cs[i]]
        exact(dx[:, a:b], R.bwd_input(gi, wts[i], H, W, k).reshape(rows, -1), f"engine dx[{i}]")
        dw, db = R.bwd_weight(gi, x4[..., a:b], k)
        exact(Ws[i].grad, dw[0].reshape(Cs[i], k * k), f"engine dw[{i}]")
        exact(Bs[i].grad, db[0], f"engine db[{i}]")
        c0 += Cs[i]
