"""The depthwise weight-gradient plans, the parts that need no GPU.  A plan entry (tc_dwconv_bwd_plan, tc_dwconv_multi_plan,
tc_ffn_mid_plan) says how many floats its launch parks and in what geometry; the engine allocates exactly that.

a. every integer the three plan entries return on a fixed grid is pinned to tests/golden/dw_plans.json, recorded from the library before the
   plan / launch geometry was gathered into one function per family;
b. the matching launch entry refuses a deferred buffer one float smaller than the plan's, before any launch -- with the GPU tests, which pass
   exactly the planned size, this pins "the launch needs exactly what the plan says"."""
import ctypes as C
import json
import os

import pytest

from transception_amd import _lib
from transception_amd._lib import TC_BF16, TC_F16, TC_F32, TcDwFold, TcDwSeg, TcFfnSeg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dw_plans.json")
DTYPES = {"f32": TC_F32, "bf16": TC_BF16, "f16": TC_F16}
FOLD_FIELDS = ("C", "k", "groups", "ch", "chunks", "gx", "nt")

# (B, H, W, C, k, groups)
SINGLE = [(2, 56, 56, 64, 3, 1), (1, 7, 7, 512, 7, 2), (1, 5, 3, 24, 5, 1), (8, 14, 14, 320, 3, 1), (16, 28, 28, 128, 3, 3),
          (4, 14, 14, 48, 5, 1), (2, 9, 9, 20, 3, 1)]
# name -> (segments as (C, k, B, H, W), groups)
_CRPE = [(16, 3, 2, 14, 14), (24, 5, 2, 14, 14), (24, 7, 2, 14, 14)]           # the relative-position triple
_MAPS = [(256, 3, 2, 56, 56), (512, 3, 2, 28, 28), (1280, 3, 2, 14, 14), (2048, 3, 2, 7, 7)]
MULTI = {"crpe_g1": (_CRPE, 1), "crpe_g3": (_CRPE, 3), "maps_g1": (_MAPS, 1)}
FFN = {"maps_g1": (_MAPS, 1), "one_g3": ([(256, 3, 2, 20, 24)], 3)}

_DUMMY = (C.c_char * 64)()
PTR = (C.addressof(_DUMMY) + 15) & ~15                             # non-null and 16-byte aligned; no entry below gets as far as reading it


def _dw_segs(segs):
    arr = (TcDwSeg * len(segs))()
    for i, (Cc, k, B, H, W) in enumerate(segs):
        arr[i] = TcDwSeg(PTR, PTR, None, PTR, PTR, PTR, PTR, Cc, k, Cc, Cc, Cc, B, H, W, None)
    return arr


def _ffn_segs(segs):
    arr = (TcFfnSeg * len(segs))()
    for i, (Cc, _, B, H, W) in enumerate(segs):
        arr[i] = TcFfnSeg(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, Cc, Cc, Cc, Cc, Cc, B, H, W, 1)
    return arr


def _site(s):
    return {f: int(getattr(s, f)) for f in FOLD_FIELDS}


def collect(L):
    """Every integer the three plan entries return on the grid, as the JSON fixture holds it."""
    out = {}
    for dn, dt in DTYPES.items():
        for case in SINGLE:
            site = TcDwFold()
            nf = int(L.tc_dwconv_bwd_plan(*case, dt, C.byref(site)))
            out[f"single/{dn}/{','.join(map(str, case))}"] = {"nf": nf, "sites": [_site(site)] if nf else []}
        for fam, plan, grid, mk in (("multi", L.tc_dwconv_multi_plan, MULTI, _dw_segs), ("ffn", L.tc_ffn_mid_plan, FFN, _ffn_segs)):
            for name, (segs, groups) in grid.items():
                n = len(segs)
                sites, offs = (TcDwFold * n)(), (C.c_longlong * n)()
                nf = int(plan(mk(segs), n, groups, dt, sites, offs))
                out[f"{fam}/{dn}/{name}"] = {"nf": nf, "sites": [_site(s) for s in sites], "offs": [int(o) for o in offs]}
    return out


@pytest.fixture(scope="module")
def L():
    from transception_amd.build import build
    build(verbose=False)
    return _lib.lib()


def test_plans_are_those_of_the_recorded_library(L):
    with open(GOLDEN) as f:
        want = json.load(f)
    got = collect(L)
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key
    # the figures the fixture was checked against when it was recorded
    s = want["single/f32/2,56,56,64,3,1"]
    assert s["nf"] == 35840 and [s["sites"][0][f] for f in ("ch", "chunks", "gx", "nt")] == [32, 2, 56, 10]
    m = want["multi/bf16/crpe_g1"]
    assert m["nf"] == 5184 and m["offs"] == [0, 320, 1984]
    for dn in ("bf16", "f16"):
        assert want[f"single/{dn}/2,9,9,20,3,1"]["nf"] == 0        # 20 channels are no multiple of the 16-bit vector


def _launches(L):
    """(key, nf, launch(ws_bytes)) for every grid case: the launch entry that parks what the plan describes."""
    with open(GOLDEN) as f:
        want = json.load(f)
    for dn, dt in DTYPES.items():
        for case in SINGLE:
            B, H, W, Cc, k, groups = case
            key = f"single/{dn}/{','.join(map(str, case))}"
            yield key, want[key]["nf"], (lambda wsb, a=(B, H, W, Cc, k), g=groups, dt=dt: L.tc_dwconv_bwd(
                PTR, a[3], PTR, a[3], PTR, PTR, a[3], PTR, PTR, *a, 0, 0, g, a[3] * a[4] * a[4], PTR, wsb, dt, None))
        for name, (segs, groups) in MULTI.items():
            key = f"multi/{dn}/{name}"
            yield key, want[key]["nf"], (lambda wsb, s=segs, g=groups, dt=dt: L.tc_dwconv_multi(
                _dw_segs(s), len(s), 3, 0, 0, g, 4096, PTR, wsb, dt, None))
        for name, (segs, groups) in FFN.items():
            key = f"ffn/{dn}/{name}"
            yield key, want[key]["nf"], (lambda wsb, s=segs, g=groups, dt=dt: L.tc_ffn_mid_bwd(
                _ffn_segs(s), len(s), g, 4096, PTR, wsb, dt, None))


def test_launch_refuses_one_float_less_than_the_plan(L):
    n = 0
    for key, nf, launch in _launches(L):
        if nf <= 0:
            continue
        with pytest.raises(_lib.TcError, match="status -1"):       # TC_ERR_ARG, raised before anything is launched
            launch(-4 * (nf - 1))
        n += 1
    assert n == 3 * (len(SINGLE) + len(MULTI) + len(FFN)) - 2      # every case but the two 16-bit ones that have no plan
