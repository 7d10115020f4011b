"""Transception: the reference's legacy network (networks/Transception.py:1010-1057) over the MI355X engine.

Encoder MiT_3inception (:362-551): the MSTransception stem and stage 1 (OverlapPatchEmbeddings + two EfficientTransformerBlocks), then
three "inception" stages of two patch-embedding branches each (a dilated 3x3 and a 1x1 convolution, stride 2), two
EfficientTransformerBlockFuse blocks over the concatenated token sets, and a fuse of the two branch maps (nearest resize of branch 1,
then conv1_1_sK or SK_Block).  Decoder: MyDecoderLayer x 4 exactly as in MSTransception, without the bridge.

Like MSTransception, the sub-modules are parameter holders only, created in the reference's constructor order with its initialisers
(same torch seed -> same weights, strict state_dict loads both ways); every operation runs as HIP kernel launches through engine.Graph,
with the nn.Module surface (forward / autograd, train / eval, compute dtype, flat arenas) inherited from MSTransception.
"""
from __future__ import annotations

from typing import List

import torch
import torch.nn as nn

from .engine import Graph, Var
from .model import (DIMS, MSTransception, _decoders, _eff_block, _lin, _ln, _mixffn_plain, _mixffn_site, _mk_decoder_layer,
                    _mk_eff_block, _mk_mixffn, _mk_mixffn_skip, _proj_ln, _sk_block)

SIZE = 224
SIDES = (56, 28, 14, 7)                      # MiT_3inception.Hs: the stage grids are hard-coded for 224 x 224 inputs (:367-368)


def _branch_geometry(dil_conv) -> tuple:
    """(k, stride, pad, dilation) of the two patch-embedding branches of stages 2-4 (Transception.py:372-397)."""
    if dil_conv:
        return (3, 2, 0, 2), (1, 2, 0, 1)
    return (3, 2, 1, 1), (1, 2, 0, 1)


# ----------------------------------------------------------------------------------------------------------
# parameter holders, built in the reference's construction order
# ----------------------------------------------------------------------------------------------------------
def _mk_patch_embed(cin: int, cout: int, k: int, stride: int, pad: int, dil: int = 1) -> nn.Module:   # OverlapPatchEmbeddings(_fuse), EffSegformer.py:117-145
    m = nn.Module()
    m.proj = nn.Conv2d(cin, cout, k, stride, pad, dil)
    m.norm = nn.LayerNorm(cout)
    return m


def _mk_fuse_block(dim: int, token_mlp: str) -> nn.Module:          # EfficientTransformerBlockFuse, Transception.py:192-210
    m = nn.Module()
    m.norm1 = nn.LayerNorm(dim)
    m.attn = nn.Module()                                            # FuseEfficientAttention, :34-43
    m.attn.keys = nn.Linear(dim, dim, bias=True)
    m.attn.queries = nn.Linear(dim, dim, bias=True)
    m.attn.values = nn.Linear(dim, dim, bias=True)
    m.attn.reprojection = nn.Linear(dim, dim)
    m.norm2 = nn.LayerNorm(dim)
    mk = _mk_mixffn if token_mlp == "mix" else _mk_mixffn_skip
    m.mlp1 = mk(dim, dim * 4)
    m.mlp2 = mk(dim, dim * 4)
    return m


def _mk_sk_block(ch: int, num_path: int = 2, reduction: int = 16, L: int = 32) -> nn.Module:   # SK_Block, Transception.py:306-327
    m = nn.Module()
    d = max(L, ch // reduction)
    m.fc = nn.Linear(ch, d)
    m.fcs = nn.ModuleList([nn.Linear(d, ch) for _ in range(num_path)])
    m.softmax = nn.Softmax(dim=0)
    m.conv_bn_ac = nn.Sequential(nn.Conv2d(ch, ch, kernel_size=(1, 1)), nn.ReLU(inplace=True), nn.BatchNorm2d(ch))
    return m


def _mk_mit_3inception(dil_conv, token_mlp: str) -> nn.Module:     # MiT_3inception.__init__, Transception.py:362-432
    m = nn.Module()
    for i, d in enumerate(DIMS):
        setattr(m, f"conv1_1_s{i + 1}", nn.Conv2d(2 * d, d, 1))
    m.patch_embed1 = _mk_patch_embed(3, DIMS[0], 7, 4, 3)
    b1, b2 = _branch_geometry(dil_conv)
    dil = 2 if dil_conv else 1                                      # the reference hands the dilation to both branches (a 1x1 ignores it)
    for s in (2, 3, 4):
        cin, cout = DIMS[s - 2], DIMS[s - 1]
        setattr(m, f"patch_embed{s}_1", _mk_patch_embed(cin, cout, b1[0], b1[1], b1[2], dil))
        setattr(m, f"patch_embed{s}_2", _mk_patch_embed(cin, cout, b2[0], b2[1], b2[2], dil))
    m.block1 = nn.ModuleList([_mk_eff_block(DIMS[0], token_mlp) for _ in range(2)])
    m.norm1 = nn.LayerNorm(DIMS[0])
    for s in (2, 3, 4):
        setattr(m, f"block{s}", nn.ModuleList([_mk_fuse_block(DIMS[s - 1], token_mlp) for _ in range(2)]))
        setattr(m, f"norm{s}", nn.LayerNorm(DIMS[s - 1]))
    for s in (2, 3, 4):
        setattr(m, f"sk_concat{s}", _mk_sk_block(DIMS[s - 1]))
    return m


class Transception(MSTransception):
    """The legacy networks/Transception.py model.  Not to be confused with `TransCeption`, this package's alias of MSTransception."""

    def __init__(self, num_classes=9, head_count=1, dil_conv=1, token_mlp_mode="mix_skip", concat='original'):
        nn.Module.__init__(self)
        # head_count reaches FuseEfficientAttention only; it must divide 64 (the gcd of 128, 320, 512), or the reference's head split breaks
        # the reprojection's shape.  token_mlp_mode: any value but "mix" / "mix_skip" builds MLP_FFN, whose forward(x, H, W) raises there.
        if not isinstance(head_count, int) or head_count <= 0 or 64 % head_count or token_mlp_mode not in ("mix_skip", "mix") or not isinstance(concat, str):
            raise NotImplementedError("Transception: implemented are head_count dividing 64, token_mlp_mode in {'mix_skip', 'mix'} and any concat string "
                                      "('original': conv1_1_sK over the concatenated branch maps, anything else: SK_Block)")
        self.num_classes, self.head_count, self.dil_conv = num_classes, head_count, dil_conv
        self.token_mlp_mode, self.concat = token_mlp_mode, concat
        self.backbone = _mk_mit_3inception(dil_conv, token_mlp_mode)
        ioc = [[32, 64, 64, 64], [144, 128, 128, 128], [288, 320, 320, 320], [512, 512, 512, 512]]
        self.decoder_3 = _mk_decoder_layer(ioc[3], num_classes, False, token_mlp_mode)
        self.decoder_2 = _mk_decoder_layer(ioc[2], num_classes, False, token_mlp_mode)
        self.decoder_1 = _mk_decoder_layer(ioc[1], num_classes, False, token_mlp_mode)
        self.decoder_0 = _mk_decoder_layer(ioc[0], num_classes, True, token_mlp_mode)
        # engine state, as MSTransception keeps it
        self.Stage_3or4, self.have_bridge, self.br_ch_att_list, self.inter = 3, "None", [False] * 4, "out"
        self.compute_dtype = torch.float32
        self.use_fused_attention = True
        self.capture_taps = False
        self.taps = {}
        self._flat = self._gflat = self._flat_lp = None
        self._lp_fresh = False
        self._index, self._uniq_params, self._used = {}, [], set()
        self.last_launches = 0

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.dim() != 4 or x.shape[1] not in (1, 3) or tuple(x.shape[2:]) != (SIZE, SIZE):
            raise ValueError(f"Transception takes [B, 1|3, 224, 224] (its stage grids are fixed, Transception.py:367-368), got {tuple(x.shape)}")
        return super().forward(x)

    def _graph_forward(self, G: Graph, x: torch.Tensor, B: int, in_ch: int, S: int) -> Var:
        if S != SIZE:
            raise ValueError(f"Transception takes 224 x 224 inputs, got {S} x {S}")
        return _forward_legacy(self, G, x, B, in_ch)

    def gradient_pieces(self):
        raise NotImplementedError("Transception: the split backward of the multi-GPU step (gradient_pieces) exists for MSTransception only; "
                                  "train this model with the single-GPU step")


# ----------------------------------------------------------------------------------------------------------
# the forward pass as engine calls
# ----------------------------------------------------------------------------------------------------------
def _patch_embed(M, G: Graph, m: Var, name: str, B: int, side: int, geo, out: Var) -> int:
    """OverlapPatchEmbeddings_fuse, EffSegformer.py:127-131: Conv2d (im2col + GEMM) + LayerNorm, written into `out`.  Returns the grid side."""
    k, s, p, d = geo
    Cin = m.cols
    if k == 1 and p == 0:
        W, b = _lin(M, G, name + ".proj")
    else:
        off, shape = M._index[name + ".proj.weight"]                     # [Cout, Cin, k, k] -> [Cout, k*k*Cin] (tap-major columns)
        W = G.permuted_weight(M._P(G, name + ".proj.weight", (shape[0], Cin * k * k)), shape[0], Cin, k * k)
        b = M._P(G, name + ".proj.bias")
    cols = G.im2col_dil(m, B, side, side, k, s, p, d)
    t = G.linear(cols, W, b)
    _ln(M, G, t, name + ".norm", out=out)
    return (side + 2 * p - d * (k - 1) - 1) // s + 1


def _fuse_attention(M, G: Graph, x: Var, name: str, B: int, n1: int, n2: int, heads: int) -> Var:
    """FuseEfficientAttention, Transception.py:45-87, on the normalised sequence x (branch-major rows: [B*n1 | B*n2]).  Its quirk: keys /
    queries / values are [b, n, d] Linear outputs REshaped (not transposed) to [b, d, n], i.e. each image's dense row-major [n, d] buffer
    is read as [d, n] -- so they are computed from a per-image copy of x ([n1 | n2] tokens of an image, branch 1 first) into one stacked
    [3, B*n, d] buffer.  Returns the attention output token-major in x's (branch-major) row order."""
    C = x.cols
    n = n1 + n2
    hk = C // heads
    xi = G.new(B * n, C)                                                # per-image token order
    G.copy_rows(x, 0, n1 * C, xi, 0, n * C, B, n1, C)
    G.copy_rows(x, B * n1 * C, n2 * C, xi, n1 * C, n * C, B, n2, C)
    kqv = G.new(3 * B * n, C, covered=True)
    Ws = [_lin(M, G, f"{name}.{p}") for p in ("keys", "queries", "values")]
    G.linear_multi(xi, [w for w, _ in Ws], [b for _, b in Ws], kqv, stacked=True)
    K, Q, V = (kqv.rowslice(i * B * n, (i + 1) * B * n).reshape(B * C, n) for i in range(3))     # [B, d, n] views of the flat buffers
    ksm = G.softmax(K, 1, 1)                                            # per (image, channel) row: over the n positions
    # the query softmax runs over the hk rows of a head, per position: on the transposed [B*n, d] view that is a row softmax over each
    # head's hk contiguous columns (the column form of tc_softmax_fwd needs n % 4 == 0; stage 4 has n = 74 or 98)
    qsm = G.softmax(G.transpose(Q, B).reshape(B * n * heads, hk), 1, 1).reshape(B * n, C)
    ctx = G.new(B * heads * hk, hk)                                     # key_h value_h^T [hk, hv]
    G.bmm(ksm, V, ctx, hk, hk, n, 0, 1, nb1=B, nb2=heads, sA=(C * n, hk * n), sB=(C * n, hk * n), sC=(heads * hk * hk, hk * hk))
    # (ctx_h^T q_h) is [hv, n]; the reference concatenates the heads to [dv, n] and permutes to [n, dv]: = q_h^T ctx_h, token-major
    o = G.new(B * n, C)
    G.bmm(qsm, ctx, o, n, hk, hk, 0, 0, nb1=B, nb2=heads, sA=(n * C, hk), sB=(heads * hk * hk, hk * hk), sC=(n * C, hk))
    ob = G.new(B * n, C)                                                # back to branch-major rows
    G.copy_rows(o, 0, n * C, ob, 0, n1 * C, B, n1, C)
    G.copy_rows(o, n1 * C, n * C, ob, B * n1 * C, n2 * C, B, n2, C)
    return ob


def _fuse_block(M, G: Graph, x: Var, name: str, B: int, g1: int, g2: int) -> Var:
    """EfficientTransformerBlockFuse, Transception.py:212-251 (x_len == n1 + n2 always holds): x + attn(norm1(x)), then per branch
    z_k + mlp_k(norm2(z_k), H_k, W_k).  norm2 is one LayerNorm for both branches, so it runs once over all rows."""
    n1, n2 = g1 * g1, g2 * g2
    r1 = B * n1
    a = _fuse_attention(M, G, _ln(M, G, x, name + ".norm1"), name + ".attn", B, n1, n2, M.head_count)
    tx, nx = _proj_ln(M, G, a, name + ".attn.reprojection", x, (name + ".norm2", 1e-5))
    out = G.new(x.rows, x.cols)
    parts = [(0, r1, g1, ".mlp1"), (r1, x.rows, g2, ".mlp2")]
    if M.token_mlp_mode == "mix":
        for a0, a1, g, mlp in parts:
            _mixffn_plain(M, G, nx.rowslice(a0, a1), name + mlp, B, g, g, tx.rowslice(a0, a1), out=out.rowslice(a0, a1))
    else:                                                               # both branches' MixFFN_skip as one site list
        G.mixffn([_mixffn_site(M, G, nx.rowslice(a0, a1), name + mlp, B, g, g, tx.rowslice(a0, a1), out.rowslice(a0, a1)) for a0, a1, g, mlp in parts])
    return out


def _inception_stage(M, G: Graph, m: Var, s: int, B: int, side: int) -> Var:
    """Stage s (2-4) of MiT_3inception.forward, Transception.py:423-505: two patch embeddings into one branch-major sequence, two fused
    blocks, normK, nearest resize of branch 1 to the branch-2 grid, fuse.  Returns the stage map token-major [B*g2*g2, C]."""
    C = DIMS[s - 1]
    bb = "backbone"
    b1, b2 = _branch_geometry(M.dil_conv)
    g1 = (side + 2 * b1[2] - b1[3] * (b1[0] - 1) - 1) // b1[1] + 1
    g2 = (side + 2 * b2[2] - b2[3] * (b2[0] - 1) - 1) // b2[1] + 1
    assert g2 == SIDES[s - 1]
    r1 = B * g1 * g1
    seq = G.new(r1 + B * g2 * g2, C, covered=True)
    _patch_embed(M, G, m, f"{bb}.patch_embed{s}_1", B, side, b1, seq.rowslice(0, r1))
    _patch_embed(M, G, m, f"{bb}.patch_embed{s}_2", B, side, b2, seq.rowslice(r1, seq.rows))
    for i in range(2):
        seq = _fuse_block(M, G, seq, f"{bb}.block{s}.{i}", B, g1, g2)
    cat = G.nearest_concat(_ln(M, G, seq, f"{bb}.norm{s}"), B, g1, g1, g2, g2, branch_major=True)
    if M.concat == "original":
        return G.linear(cat, *_lin(M, G, f"{bb}.conv1_1_s{s}"))
    return _sk_block(M, G, cat, f"{bb}.sk_concat{s}", B, g2 * g2, C)


def _forward_legacy(M: Transception, G: Graph, x: torch.Tensor, B: int, in_ch: int) -> Var:
    """Transception.forward, Transception.py:1036-1055 (MiT_3inception.forward, :434-551)."""
    S = SIZE
    G.segment("stage1")
    cols = G.stem_im2col(x, B, in_ch, S, S)                          # x.repeat(1, 3, 1, 1) of a 1-channel input folded in
    t = G.linear(cols.colslice(0, 147), *_lin(M, G, "backbone.patch_embed1.proj"))
    t = _ln(M, G, t, "backbone.patch_embed1.norm")
    for i in range(2):
        t = _eff_block(M, G, t, f"backbone.block1.{i}", B, SIDES[0], SIDES[0])
    maps: List[Var] = [_ln(M, G, t, "backbone.norm1")]
    for s in (2, 3, 4):
        G.segment(f"stage{s}")
        maps.append(_inception_stage(M, G, maps[-1], s, B, SIDES[s - 2]))
    G.mark("encoder_done")
    return _decoders(M, G, maps, B, list(SIDES), False)
