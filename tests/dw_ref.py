"""Host reference of the depthwise convolutions of csrc/dwconv.hip (include/transception_hip.h: tc_dwconv_fwd, tc_dwconv_bwd_input,
tc_dwconv_bwd_weight, tc_dwconv_bwd, tc_dwconv_multi, tc_ffn_dw_fwd, tc_dw_fold), in float64 on CPU tensors, with the inputs, the buffers and
the case lists of tests/test_dwconv_abi_gpu.py.  tests/test_dw_ref_host.py holds the reference to torch.nn.functional.conv2d and its autograd
and checks that every case below keeps its arithmetic exact.

The reference is the definition written out: a loop over the k x k taps, each tap a zero-padded shift of the whole NHWC map ("shift and add").
Maps are [groups * B, H, W, C] tensors: `groups` stacked sets of B images, set g convolved with the filters w[g] ([groups, C, k, k]) and the bias
b[g] ([groups, C]) -- in device memory the parameters of set g stand g * wstride elements behind those of set 0 (`Params`).

Exactness rule (as tests/gemm_ref.py, tests/test_gate_kernels_gpu.py): map values are multiples of 1/2 with |v| <= 2, weights and biases multiples
of 1/4 with |v| <= 1.  A forward product is a multiple of 1/8, a weight-gradient product a multiple of 1/4; as long as sum|term| / quantum < 2^24
every fp32 partial sum is exact whatever the order, and the only rounding is the store (`premise`)."""
import zlib

import torch

SENT = -96.0                       # exact in every storage type, never a result of the grids below
NAN = float("nan")
KS = (3, 5, 7)
CGS = (2, 4, 8)


# ---------------------------------------------------------------------------------------------------------------- the reference
def _shift(t, dy, dx):
    """t [N, H, W, C] -> s with s[n, y, x] = t[n, y + dy, x + dx], zero outside the map."""
    H, W = t.shape[1:3]
    out = torch.zeros_like(t)
    ys, ye, xs, xe = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[:, ys:ye, xs:xe] = t[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def out_hw(H, W, k, stride):
    """Output extent with padding (k - 1) / 2."""
    P = (k - 1) // 2
    return (H + 2 * P - k) // stride + 1, (W + 2 * P - k) // stride + 1


def _per_image(p, groups, N):
    """[groups, C, ...] parameters -> [N, 1, 1, C, ...]: image n belongs to set n // (N / groups)."""
    B = N // groups
    assert B * groups == N
    idx = torch.arange(N) // B
    return p.double()[idx][:, None, None]


def fwd(x, w, bias, k, stride=1, add_input=False, groups=1):
    """y[n, oh, ow, c] = bias[c] + sum_taps w[c, ky, kx] x[n, oh s + ky - P, ow s + kx - P, c] (+ x[n, oh, ow, c], stride 1)."""
    x, P = x.double(), (k - 1) // 2
    N, H, W, C = x.shape
    wi = _per_image(w.reshape(groups, C, k, k), groups, N)                   # [N, 1, 1, C, k, k]
    Ho, Wo = out_hw(H, W, k, stride)
    y = torch.zeros(N, Ho, Wo, C, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            y += wi[..., ky, kx] * _shift(x, ky - P, kx - P)[:, ::stride, ::stride]
    if bias is not None:
        y += _per_image(bias.reshape(groups, C), groups, N)
    if add_input:
        assert stride == 1
        y += x
    return y


def bwd_input(dy, w, H, W, k, stride=1, add_input=False, groups=1):
    """dx[n, ih, iw, c] = sum over the (oh, ow, ky, kx) with oh s + ky - P == ih, ow s + kx - P == iw of w[c, ky, kx] dy[n, oh, ow, c] (+ dy)."""
    dy, P = dy.double(), (k - 1) // 2
    N, Ho, Wo, C = dy.shape
    assert (Ho, Wo) == out_hw(H, W, k, stride)
    wi = _per_image(w.reshape(groups, C, k, k), groups, N)
    up = torch.zeros(N, H, W, C, dtype=torch.float64)                        # dy on the input grid: output (oh, ow) sits at (oh s, ow s)
    up[:, ::stride, ::stride] = dy
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            dx += wi[..., ky, kx] * _shift(up, P - ky, P - kx)
    if add_input:
        assert stride == 1
        dx += dy
    return dx


def bwd_weight(dy, x, k, stride=1, groups=1):
    """(dw [groups, C, k, k], db [groups, C]): dw[g, c, ky, kx] = sum over set g's pixels of dy[n, oh, ow, c] x[n, oh s + ky - P, ow s + kx - P, c]."""
    dy, x, P = dy.double(), x.double(), (k - 1) // 2
    N, H, W, C = x.shape
    B = N // groups
    dw = torch.zeros(groups, C, k, k, dtype=torch.float64)
    for ky in range(k):
        for kx in range(k):
            prod = dy * _shift(x, ky - P, kx - P)[:, ::stride, ::stride]
            dw[:, :, ky, kx] = prod.reshape(groups, B, -1, C).sum(dim=(1, 2))
    return dw, dy.reshape(groups, B, -1, C).sum(dim=(1, 2))


def chunk_stats(y, ch):
    """[..., C] -> [..., C / ch, 2]: per pixel and chunk of ch channels, (sum, sum of squared deviations from the chunk mean)."""
    y = y.double()
    C = y.shape[-1]
    assert C % ch == 0
    v = y.reshape(*y.shape[:-1], C // ch, ch)
    s = v.sum(dim=-1)
    return torch.stack([s, ((v - s[..., None] / ch) ** 2).sum(dim=-1)], -1)


def fold(part, C, kk, ch, chunks, gx, nt, groups):
    """tc_dw_fold's sums of one site: part [groups * chunks][gx][nt][ch] -> [groups, nt, C] float64 (taps 0 .. kk - 1 the filter's, kk the
    bias's, kk + 1 / kk + 2 dgamma's / dbeta's); the channels a last chunk has past C belong to nobody."""
    p = part.double().reshape(groups, chunks, gx, nt, ch).sum(dim=2)         # [groups, chunks, nt, ch]
    return p.permute(0, 2, 1, 3).reshape(groups, nt, chunks * ch)[:, :, :C]


# ---------------------------------------------------------------------------------------------------------------- dispatcher geometry, restated
def vec_of(dtype):
    """Channels per 16 bytes."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def pick_cg(C, vec):
    """dw_pick_cg: 16-byte lanes per pixel that waste the fewest channels (ties: the widest)."""
    best, waste = 8, -(-C // (8 * vec)) * 8 * vec - C
    for cg in (4, 2):
        w = -(-C // (cg * vec)) * cg * vec - C
        if w < waste:
            best, waste = cg, w
    return best


def tile_geom(B, H, W, C, vec):
    """(cg, ch, chunks, TH, ntiles) of the tile kernels: TH x 16 pixel tiles, TH = 32 / 16 / 8 for cg = 2 / 4 / 8."""
    cg = pick_cg(C, vec)
    TH = 64 // cg
    return cg, cg * vec, -(-C // (cg * vec)), TH, B * (-(-W // 16)) * (-(-H // TH))


def walkers(B, H, W, C, groups, vec):
    """dw_bwd_layout: walkers per (group, chunk) of tc_dwconv_bwd / tc_dwconv_bwd_weight: 512 / (chunks * groups), at most one per tile, at least 1."""
    _, _, chunks, _, ntiles = tile_geom(B, H, W, C, vec)
    return max(1, min(512 // (chunks * groups), ntiles))


# ---------------------------------------------------------------------------------------------------------------- inputs and buffers
def _gen(tag):
    return torch.Generator().manual_seed(zlib.crc32(tag.encode()))


def halves(tag, shape, dtype=torch.float32, lim=4):
    """Seeded multiples of 1/2 with |v| <= lim / 2 (no -0.0)."""
    return (torch.randint(-lim, lim + 1, shape, generator=_gen("h/" + tag)).float() / 2).to(dtype)


def quarters(tag, shape, dtype=torch.float32):
    """Seeded multiples of 1/4 with |v| <= 1."""
    return (torch.randint(-4, 5, shape, generator=_gen("q/" + tag)).float() / 4).to(dtype)


class Map:
    """An operand in an oversize buffer: `lead` elements, then rows + spare rows of ld elements; the operand is rows x C at the top left.
    Inputs are NaN outside the operand (one read out of range poisons a result), outputs hold the sentinel, or grid values where the
    entry adds to what is there."""

    def __init__(self, flat, lead, rows, C, ld):
        self.flat, self.lead, self.rows, self.C, self.ld = flat, lead, rows, C, ld

    def logical(self, flat=None):
        f = self.flat if flat is None else flat
        return f[self.lead:].as_strided((self.rows, self.C), (self.ld, 1))

    def write(self, out64, val64, accumulate=False):
        """val64 ([rows, C] or anything of that many elements) written to, or added into, the operand's place in out64 (a float64 copy of flat)."""
        v = val64.reshape(self.rows, self.C)
        tgt = self.logical(out64)
        tgt.copy_(tgt + v if accumulate else v)
        return out64

    def expect(self, val64, accumulate=False):
        """The whole buffer expected after the call, float64."""
        return self.write(self.flat.double().clone(), val64, accumulate)

    def cols(self, off, C):
        """Columns off : off + C of the operand as an operand of its own in the same storage (a channel slice of a wider map)."""
        return Map(self.flat, self.lead + off, self.rows, C, self.ld)


def in_map(tag, rows, C, ld, dtype, lead=0, spare=1):
    flat = torch.full((lead + (rows + spare) * ld,), NAN, dtype=dtype)
    m = Map(flat, lead, rows, C, ld)
    m.logical().copy_(halves(tag, (rows, C), dtype))
    return m


def out_map(tag, rows, C, ld, dtype, acc=False, lead=0, spare=2):
    flat = torch.full((lead + (rows + spare) * ld,), SENT, dtype=dtype)
    m = Map(flat, lead, rows, C, ld)
    if acc:
        m.logical().copy_(halves(tag, (rows, C), dtype))
    return m


class Params:
    """Per-group parameter blocks of n elements each, group g at + g * wstride of a flat buffer; `fill` between and behind the blocks (NaN for
    an input, the sentinel for a += target, whose blocks start from grid values)."""

    def __init__(self, tag, n, groups, wstride, dtype, gen, fill):
        assert groups == 1 or wstride >= n
        self.n, self.groups, self.wstride = n, groups, wstride
        self.flat = torch.full(((groups - 1) * wstride + n + 2,), fill, dtype=dtype)
        for g in range(groups):
            self.flat[g * wstride:g * wstride + n] = gen(f"{tag}/{g}", (n,), dtype)

    def blocks(self, flat=None):
        f = self.flat if flat is None else flat
        return torch.stack([f[g * self.wstride:g * self.wstride + self.n] for g in range(self.groups)])      # [groups, n]

    def expect_add(self, val64):
        """The whole buffer after `+= val64` ([groups, n]), float64."""
        out = self.flat.double().clone()
        for g in range(self.groups):
            out[g * self.wstride:g * self.wstride + self.n] += val64[g].reshape(-1)
        return out


class Prob:
    """One depthwise convolution with every operand of its three directions, laid out for the C ABI.
    ld = C + pad * unit for x, y, dy, dx with pad = 1, 2, 3, 4 (all different, all larger than C); lead[name] elements in front of a buffer
    move its base off the 16-byte grid; the parameters of group g stand wstride = C k k + gap behind group 0's."""

    def __init__(self, tag, dtype, B, H, W, C, k, stride=1, groups=1, unit=None, lead=None, gap=12, wstride=None):
        self.tag, self.dtype, self.B, self.H, self.W, self.C, self.k, self.stride, self.groups = tag, dtype, B, H, W, C, k, stride, groups
        unit = unit or vec_of(dtype)
        lead = lead or {}
        self.Ho, self.Wo = out_hw(H, W, k, stride)
        N = groups * B
        self.rin, self.rout = N * H * W, N * self.Ho * self.Wo
        self.ld = {n: C + (i + 1) * unit for i, n in enumerate(("x", "y", "dy", "dx"))}
        self.x = in_map(tag + "/x", self.rin, C, self.ld["x"], dtype, lead.get("x", 0))
        self.dy = in_map(tag + "/dy", self.rout, C, self.ld["dy"], dtype, lead.get("dy", 0))
        self.lead = lead
        self.wstride = wstride or C * k * k + gap
        self.w = Params(tag + "/w", C * k * k, groups, self.wstride, dtype, quarters, NAN)
        self.b = Params(tag + "/b", C, groups, self.wstride, dtype, quarters, NAN)
        self._ref = {}

    # operands as the reference takes them
    def x4(self):
        return self.x.logical().reshape(self.groups * self.B, self.H, self.W, self.C)

    def dy4(self):
        return self.dy.logical().reshape(self.groups * self.B, self.Ho, self.Wo, self.C)

    def w4(self):
        return self.w.blocks().reshape(self.groups, self.C, self.k, self.k)

    def b2(self):
        return self.b.blocks()

    # output buffers before the call
    def y0(self, acc=False):
        return out_map(self.tag + "/y0", self.rout, self.C, self.ld["y"], self.dtype, acc, self.lead.get("y", 0))

    def dx0(self, acc=False):
        return out_map(self.tag + "/dx0", self.rin, self.C, self.ld["dx"], self.dtype, acc, self.lead.get("dx", 0))

    def dw0(self):
        return Params(self.tag + "/dw0", self.C * self.k * self.k, self.groups, self.wstride, torch.float32, halves, SENT)

    def db0(self):
        return Params(self.tag + "/db0", self.C, self.groups, self.wstride, torch.float32, halves, SENT)

    # float64 references (computed once)
    def _cached(self, key, fn):
        if key not in self._ref:
            self._ref[key] = fn()
        return self._ref[key]

    def ref_fwd(self, bias, add):
        base = self._cached("fwd", lambda: fwd(self.x4(), self.w4(), None, self.k, self.stride, False, self.groups))
        y = base.clone()
        if bias:
            y += _per_image(self.b2(), self.groups, y.shape[0])
        return y + self.x4().double() if add else y

    def ref_bwd_input(self, add):
        base = self._cached("bwi", lambda: bwd_input(self.dy4(), self.w4(), self.H, self.W, self.k, self.stride, False, self.groups))
        return base + self.dy4().double() if add else base

    def ref_bwd_weight(self):
        return self._cached("bww", lambda: bwd_weight(self.dy4(), self.x4(), self.k, self.stride, self.groups))

    def premise(self):
        """sum|term| / quantum < 2^24 for each of the three reductions, the += targets' and the accumulated outputs' old values included (every
        test asserts this before it launches; tests/test_dw_ref_host.py asserts it for every case without a GPU)."""
        ax, ady, aw, ab = self.x4().abs(), self.dy4().abs(), self.w4().abs(), self.b2().abs()
        lim = 2.0 ** 24
        f = fwd(ax, aw, ab, self.k, self.stride, self.stride == 1, self.groups) + 2.0          # + |y0| <= 2
        i = bwd_input(ady, aw, self.H, self.W, self.k, self.stride, self.stride == 1, self.groups) + 2.0
        dw, db = bwd_weight(ady, ax, self.k, self.stride, self.groups)
        assert float(f.max()) / 0.125 < lim and float(i.max()) / 0.125 < lim, self.tag
        assert (float(dw.max()) + 2.0) / 0.25 < lim and (float(db.max()) + 2.0) / 0.5 < lim, self.tag
        for t in (self.x.logical(), self.dy.logical()):                       # the grids themselves
            assert bool(((t.double() * 2) % 1 == 0).all()) and float(t.abs().max()) <= 2.0, self.tag
        for t in (self.w.blocks(), self.b.blocks()):
            assert bool(((t.double() * 4) % 1 == 0).all()) and float(t.abs().max()) <= 1.0, self.tag
        return True


def is_f32_value(t64):
    """Nothing rounds before the store: the float64 reference is a float32 value."""
    return torch.equal(t64.float().double(), t64)


# ---------------------------------------------------------------------------------------------------------------- the cases of test_dwconv_abi_gpu.py
def c_for_cg(cg, vec):
    """The narrowest C for which dw_pick_cg returns cg: one full chunk (fp32 8 / 16 / 32, 16-bit 16 / 32 / 64)."""
    return cg * vec


def edge_maps(cg):
    """(B, H, W, groups): the smallest maps with a first, an interior and a last partial tile in both directions of TH x 16 tiles: 1 x 1, H < k,
    W < k, W = 5 / 16 / 17 / 18, H = TH - 1 / TH / TH + 1, B = 1 and 3, groups 1 and 2."""
    TH = 64 // cg
    return [(1, 1, 1, 1), (1, 2, 5, 2), (3, TH - 1, 16, 1), (1, TH, 18, 1), (3, TH + 1, 17, 2), (1, TH + 1, 2, 1)]


def chunk_cs(vec):
    """(C, cg, chunks, last chunk partial): a partial last chunk for each cg and several chunks (fp32 20 / 12 / 28 / 96 / 48, 16-bit twice that)."""
    u = vec // 4
    return [(20 * u, 2, 3, True), (12 * u, 4, 1, True), (28 * u, 8, 1, True), (96 * u, 8, 3, False), (48 * u, 4, 3, False)]


# 16-bit only: why the dispatcher leaves the tile kernels (dw_tile_ok false) -> (C, unit of the ld paddings, lead elements per operand)
STRIP_WHY = {
    "C%8==4": dict(C=12, unit=4, lead={}),                                  # ld = 16 / 20 / 24 / 28: the channel count alone decides
    "C=68": dict(C=68, unit=4, lead={}),                                    # two 64-channel blocks, the second with 4 channels
    "ld%8==4": dict(C=16, unit=4, lead={}),                                 # ldx = 20, lddy = 28
    "base%16==8": dict(C=16, unit=8, lead={"x": 4, "dy": 4}),                # every ld a multiple of 8; x and dy 8 bytes off the 16-byte grid
    "out base%16==8": dict(C=16, unit=8, lead={"y": 4, "dx": 4}),            # the written operand 8 bytes off
}
# (B, H, W, groups) per k: W >= 2 (k + 1) splits a row into W-segments (nseg = W / (k + 1) on these small maps), W = 9 / 13 / 17 is not divided by
# its 2 segments; the 1 x 1 map and W < k have one segment
STRIP_MAPS = {3: [(2, 3, 9, 1), (1, 2, 13, 2), (1, 1, 1, 1), (1, 4, 2, 1)], 5: [(2, 3, 13, 1), (1, 2, 19, 2), (1, 1, 1, 1), (1, 6, 4, 1)],
              7: [(2, 3, 17, 1), (1, 2, 25, 2), (1, 1, 1, 1), (1, 8, 6, 1)]}


def strip_nseg(B, H, W, C, k, groups):
    """launch_strip's W-segments per row."""
    cpt = 4 if k == 3 else 2
    nseg = 262144 // (B * H * groups * (-(-C // cpt)))
    return max(1, min(nseg, max(1, W // (k + 1))))


# stride 2: (B, H, W): odd and even extents, H != W, maps smaller than the filter
STRIDE2_MAPS = [(2, 7, 10), (1, 8, 5), (1, 1, 1), (1, 2, 3)]
STRIDE2_CS = (8, 68)                                                        # one partial 64-channel block; two blocks, the second partial


def walker_cases(vec):
    """name -> (B, H, W, C, k, groups) of the weight-gradient tail cases; the premise of each (walkers gx against tiles) is asserted by
    walker_premise from tc_dwconv_bwd_plan."""
    return {
        # cg 8 (8 x 16 tiles), 3 chunks, 2 groups: 512 / 6 = 85 walkers on 92 tiles, 7 of them visit two.  fp32: 23 maps of 9 x 17 (4 tiles each,
        # 0.7 M elements); 16-bit, with twice the channels: 46 maps of 9 x 5 (2 tiles each, 0.8 M elements)
        "gx<ntiles": (23, 9, 17, 24 * vec, 3, 2) if vec == 4 else (46, 9, 5, 24 * vec, 3, 2),
        "gx%4!=0": (3, 17, 17, 8 * vec, 5, 1),         # cg 8, TH 8: 3 * 2 * 3 = 18 tiles = 18 walkers: arrival groups of 4, 4, 4, 4, 2
        "gx==3": (1, 17, 16, 8 * vec, 7, 2),           # 3 tiles: one short group only
        "gx==1": (1, 5, 7, 4 * vec, 3, 1),             # one tile, one walker: nothing parked, nothing counted
    }


def walker_premise(name, gx, ntiles):
    return {"gx<ntiles": gx < ntiles and ntiles % gx != 0 and gx > 32 and gx % 32 != 0, "gx%4!=0": gx > 4 and gx % 4 != 0, "gx==3": gx == 3,
            "gx==1": gx == 1}[name]


def ffn_cases(vec):
    """(C, groups) of the tc_ffn_dw_fwd cases: two chunks of cg 8, one of cg 4 on two groups, one of cg 2 (chunk widths 8 / 4 / 2 vectors: powers of two)."""
    return [(16 * vec, 1), (4 * vec, 2), (2 * vec, 1)]


MULTI_WSTRIDE = 1200                                                        # one parameter stride for every segment of a launch (>= 24 * 49)


def multi_cases(dtype):
    """name -> (list of Prob, wide): the segments of the tc_dwconv_multi cases.  wide: column slices of ONE map per operand (the crpe layout);
    else every segment in buffers of its own.
      crpe g1 / g3: k = 3 / 5 / 7 on 2 / 3 / 3 vectors of channels of one 2 x 5 x 18 map (cg 2, and cg 4 with a partial chunk); one launch;
      maps        : different maps, channel counts and k per segment; one launch;
      fallback    : (16-bit) the second segment has ld % 8 == 4 for x and dy -> every segment through the single entries."""
    vec, dn = vec_of(dtype), _dn(dtype)

    def mk(name, i, B, H, W, C, k, G, unit=None):
        return _memo(("multi", dtype, name, i), lambda: Prob(f"multi/{dn}/{name}/{i}", dtype, B, H, W, C, k, 1, G, unit, None, 12, MULTI_WSTRIDE))
    out = {}
    for G in (1, 3):
        out[f"crpe g{G}"] = ([mk(f"crpe{G}", i, 2, 5, 18, c * vec, k, G) for i, (c, k) in enumerate(((2, 3), (3, 5), (3, 7)))], True)
    out["maps"] = ([mk("maps", 0, 1, 9, 17, 4 * vec, 7, 1), mk("maps", 1, 2, 3, 5, 2 * vec, 3, 1), mk("maps", 2, 1, 1, 1, vec, 5, 1),
                    mk("maps", 3, 1, 17, 4, 8 * vec, 3, 1)], False)
    if dtype != torch.float32:
        out["fallback"] = ([mk("fb", 0, 2, 5, 9, 16, 3, 1, 8), mk("fb", 1, 1, 4, 13, 24, 5, 1, 4)], False)
        out["fallback g3"] = ([mk("fb3", 0, 1, 5, 9, 16, 7, 3, 8), mk("fb3", 1, 1, 4, 9, 24, 3, 3, 4)], False)
    return out


def all_probs(dtype):
    """Every Prob the GPU file builds for this dtype (name, Prob): the host test asserts the premise of each."""
    vec = vec_of(dtype)
    for k in KS:
        for cg in CGS:
            for m in edge_maps(cg):
                yield tile_prob(dtype, k, cg, m)
    for C, *_ in chunk_cs(vec):
        for k in KS:
            yield chunk_prob(dtype, C, k)
    if dtype != torch.float32:
        for why in STRIP_WHY:
            for k in KS:
                for m in STRIP_MAPS[k]:
                    yield strip_prob(dtype, why, k, m)
    for C in STRIDE2_CS:
        for k in KS:
            for m in STRIDE2_MAPS:
                yield stride2_prob(dtype, C, k, m)
    for name in walker_cases(vec):
        yield walker_prob(dtype, name)
    for C, G in ffn_cases(vec):
        yield ffn_prob(dtype, C, G)
    for probs, _ in multi_cases(dtype).values():
        yield from probs


_PROBS = {}


def _memo(key, make):
    """Inputs and references are built once and shared by the tests that use them (nothing writes to them)."""
    if key not in _PROBS:
        _PROBS[key] = make()
    return _PROBS[key]


def _dn(dtype):
    return str(dtype).split(".")[-1]


def tile_prob(dtype, k, cg, m):
    B, H, W, G = m
    C = c_for_cg(cg, vec_of(dtype))
    return _memo(("tile", dtype, k, cg, m), lambda: Prob(f"tile/{_dn(dtype)}/{k}/{cg}/{m}", dtype, B, H, W, C, k, 1, G))


def chunk_prob(dtype, C, k):
    return _memo(("chunk", dtype, C, k), lambda: Prob(f"chunk/{_dn(dtype)}/{C}/{k}", dtype, 2, 9, 19, C, k, 1, 1))


def strip_prob(dtype, why, k, m):
    B, H, W, G = m
    s = STRIP_WHY[why]
    return _memo(("strip", dtype, why, k, m), lambda: Prob(f"strip/{_dn(dtype)}/{why}/{k}/{m}", dtype, B, H, W, s["C"], k, 1, G, s["unit"], s["lead"]))


def stride2_prob(dtype, C, k, m):
    B, H, W = m
    return _memo(("s2", dtype, C, k, m), lambda: Prob(f"s2/{_dn(dtype)}/{C}/{k}/{m}", dtype, B, H, W, C, k, 2, 1))


def walker_prob(dtype, name):
    B, H, W, C, k, G = walker_cases(vec_of(dtype))[name]
    return _memo(("walk", dtype, name), lambda: Prob(f"walk/{_dn(dtype)}/{name}", dtype, B, H, W, C, k, 1, G))


def ffn_prob(dtype, C, G):
    return _memo(("ffn", dtype, C, G), lambda: Prob(f"ffn/{_dn(dtype)}/{C}/{G}", dtype, 2, 9, 18, C, 3, 1, G))
