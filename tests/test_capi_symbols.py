"""The C-ABI library loads without a GPU and exports every symbol include/transception_hip.h declares; the ctypes
binding (transception_amd/_lib.py, derived from the header by _header.py) agrees with the header on every argument count, with a
C compiler on every struct layout, and checks the status of every entry that returns one.  No compute calls here."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "transception_hip.h")


def header_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    struct = re.search(r"typedef struct TcGemm \{(.*?)\} TcGemm;", src, flags=re.S).group(1)
    src = src.replace(struct, "")
    fns = {}
    for m in re.finditer(r"\b(?:int|long long)\s+(tc_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2).strip()
        fns[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    nfields = sum(len([x for x in decl.split(",") if x.strip()]) for decl in
                  re.findall(r"(?:const void\*|void\*|float\*|int|long long|float)\s+([^;]+);", struct))
    return fns, nfields


@pytest.fixture(scope="module")
def built():
    from transception_amd.build import build
    return build(verbose=False)


def test_library_exports_every_declared_symbol(built):
    fns, _ = header_functions()
    assert len(fns) >= 30
    dll = ctypes.CDLL(built)
    for name in fns:
        assert hasattr(dll, name), f"{name} declared in the header but not exported by {built}"
    from transception_amd import _lib
    assert dll.tc_abi_version() == _lib.ABI_VERSION == 15


def test_ctypes_binding_matches_header(built):
    from transception_amd import _lib
    fns, nfields = header_functions()
    assert set(_lib.SIGNATURES) == set(fns), set(_lib.SIGNATURES) ^ set(fns)
    for name, n in fns.items():
        assert len(_lib.SIGNATURES[name]) == n, f"{name}: header has {n} args, ctypes binding {len(_lib.SIGNATURES[name])}"
    assert len(_lib.TcGemm._fields_) == nfields
    assert _lib.lib().tc_bn_scratch_floats(1000, 64) == 64 * (1 + 2 * 16)


def test_missing_library_fails_loudly(tmp_path):
    from transception_amd import _lib
    with pytest.raises(_lib.TcError):
        _lib._Lib(str(tmp_path / "nope.so"))


# ---- the binding is derived from the header (transception_amd/_header.py): hold the parser to the header, a C compiler and the library

QUERIES = {"tc_abi_version",
           "tc_ln_cls_supported", "tc_linear_ln_supported", "tc_ripm_supported", "tc_mhca_att_supported", "tc_dw_ln_supported",
           "tc_mhca_att_bwd_supported", "tc_effatt_supported", "tc_ffn_fused_supported", "tc_ffn_fused_bwd_supported",
           "tc_ripm_tiles", "tc_ffn_chunk", "tc_layernorm_bwd_nblk",
           "tc_ln_cls_scratch_floats", "tc_effatt_scratch_floats", "tc_ffn_fused_bwd_scratch_floats", "tc_bn_scratch_floats",
           "tc_softmax_scratch_floats", "tc_layernorm_bwd_scratch_floats", "tc_dwconv_bwd_plan", "tc_dwconv_multi_plan", "tc_ffn_mid_plan",
           "tc_factor_att_stats_floats", "tc_metric_hist_bins"}


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from transception_amd import _lib
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    structs = _lib.ABI.structs
    assert len(structs) == 10
    lines = ["#include <stdio.h>", "#include <stddef.h>", f'#include "{HEADER}"', "int main(void) {"]
    for name, cls in structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _ in cls._fields_]
    (tmp_path / "layout.c").write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run([cc, "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    theirs = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    ours = {}
    for name, cls in structs.items():
        ours[name] = ctypes.sizeof(cls)
        ours.update({f"{name}.{f}": getattr(cls, f).offset for f, _ in cls._fields_})
    assert len(ours) == 10 + sum(len(cls._fields_) for cls in structs.values())
    assert ours == theirs


def test_no_declaration_is_skipped():
    from transception_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    src = re.sub(r"\{[^{}]*\}", "", src)                  # struct (and enum) bodies
    assert len(re.findall(r"\btc_\w+\s*\(", src)) == len(_lib.SIGNATURES) == 137


def test_status_entries_are_checked_and_queries_raw(built):
    from transception_amd import _lib
    L, fns = _lib.lib(), _lib.ABI.functions
    assert {n for n, f in fns.items() if f.query} == QUERIES and len(QUERIES) == 24
    for name, f in fns.items():
        entry = getattr(L, name)
        if f.query:
            assert entry is getattr(L.cdll, name) and entry.restype is f.restype, name          # exposed raw
        else:
            assert f.restype is ctypes.c_int and getattr(L.cdll, name).restype is ctypes.c_int, name
            assert entry.__name__ == name and entry is not getattr(L.cdll, name), name           # wrapped by _Lib._checked
        if f.restype is not ctypes.c_int:
            assert f.restype is ctypes.c_longlong and f.query, name                               # every long long return is a query
        assert getattr(L.cdll, name).argtypes == f.argtypes == _lib.SIGNATURES[name], name
    # what the wrapper does with a status: it counts the call, passes 0 and raises on anything else
    calls0 = _lib._Lib.calls
    assert _lib._Lib._checked("tc_ok", lambda *a: 0)(1, 2) is None and _lib._Lib.calls == calls0 + 1
    with pytest.raises(_lib.TcError, match="tc_bad failed with status -3"):
        _lib._Lib._checked("tc_bad", lambda *a: -3)()
    with pytest.raises(_lib.TcError, match="status -1"):                     # a real status entry: null arguments, refused before any launch
        L.tc_metric_select(None, 0, 0, None, None)


def test_pinned_types():
    from transception_amd import _lib
    S, vp = _lib.SIGNATURES, ctypes.c_void_p
    assert S["tc_adam_step_multi"][10:12] == [ctypes.c_double] * 2 and S["tc_adam_advance"][2:4] == [ctypes.c_double] * 2
    assert S["tc_dropout"][5] is ctypes.c_uint
    assert dict(_lib.TcSliceAug._fields_)["m"] is ctypes.c_double * 6
    assert S["tc_gemm"] == [vp, vp]
    assert all(t in (vp, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_double, ctypes.c_uint) for a in S.values() for t in a)


def test_parser_refuses_what_it_does_not_understand():
    from transception_amd import _header
    text = open(HEADER).read()
    assert len(_header.parse(text).functions) == 137
    anchor = "int tc_gemm(const TcGemm* g, void* stream);"
    assert text.count(anchor) == 1
    for bad in (anchor.replace("void* stream", "size_t n, void* stream"),      # an unknown scalar type
                anchor.replace("const TcGemm*", "const TcNoSuch*"),             # a pointer to an unknown type
                anchor + "\nstatic",                                            # a stray token between two declarations
                anchor + "\n;",
                anchor.replace(");", ";"),                                      # a declaration that does not balance
                anchor + "\nlong long tc_new_floats(int n);",                   # a value-returning entry without TC_QUERY
                anchor + "\n#define TC_NEW (1 * 2)",                            # outside the constant grammar
                anchor + "\n#include <stddef.h>"):
        with pytest.raises(_header.HeaderError):
            _header.parse(text.replace(anchor, bad))
    for expr in ("__import__('os')", "1 <<", "(1", "2 ** 3", "0x10", "TC_OK"):
        with pytest.raises(_header.HeaderError):
            _header.evaluate(expr)
    assert _header.evaluate("(-2147483647 - 1)") == -2 ** 31 and _header.evaluate("1 << 20 | (3 + 4)") == (1 << 20) | 7


def test_constants_come_from_the_header(built):
    from transception_amd import _lib, train
    assert _lib.TC_IGNORE_NONE == train.IGNORE_NONE == -2 ** 31
    assert _lib.TC_METRIC_NO_SOURCE == 1 << 28
    assert _lib.TC_AUG_FROM_RAW == 1 << 21
    assert _lib.ABI_VERSION == ctypes.CDLL(built).tc_abi_version() == 15
    assert (_lib.TC_F32, _lib.TC_BF16, _lib.TC_F16, _lib.ACT_GELU, _lib.FFN_EP, _lib.EW_COPY, _lib.EW_MULTI_MAX, _lib.ATTN_DKV_SPLITS,
            _lib.TC_AUG_PIECEWISE, _lib.TC_AUG_SKIP, _lib.TC_METRIC_SELECT_WORK_BYTES) == (0, 1, 2, 4, 3, 2, 4, 8, 8, 1 << 20, 16448)
