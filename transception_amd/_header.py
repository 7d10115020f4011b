"""Reads include/transception_hip.h, the one place where the C ABI is written, into what a ctypes binding needs:
the functions (restype, argtypes, status or TC_QUERY), the structs and the constants.

The parser knows the subset of C the header uses and refuses everything else: an unknown type, a declaration that does not
balance or any text it cannot account for raises HeaderError, so the binding can never quietly skip part of the ABI.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
import re
from typing import NamedTuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "transception_hip.h")


class SideHeader(NamedTuple):
    """A part of the C ABI that replaces no reference call site and so has a header and a version of its own."""
    attr: str                 # the name _lib.py gives the parsed header
    file: str                 # beside HEADER
    version: str              # the constant that holds the host's version
    entry: str                # the TC_QUERY entry that returns the library's
    what: str                 # how a mismatch names it

    @property
    def path(self) -> str:
        return os.path.join(os.path.dirname(HEADER), self.file)


# read by _lib.py (load, bind, version check) and by build.py (staleness): a new side header is one line here
SIDE_HEADERS = (SideHeader("POST", "transception_post.h", "TC_POST_ABI_VERSION", "tc_post_abi_version", "post-processing"),
                SideHeader("EMA", "transception_ema.h", "TC_EMA_ABI_VERSION", "tc_ema_abi_version", "weight-averaging"),
                SideHeader("TTA", "transception_tta.h", "TC_TTA_ABI_VERSION", "tc_tta_abi_version", "test-time augmentation"),
                SideHeader("RESAMPLE", "transception_resample.h", "TC_RESAMPLE_ABI_VERSION", "tc_resample_abi_version", "score resampling"),
                SideHeader("BRIDGE", "transception_bridge.h", "TC_BRIDGE_ABI_VERSION", "tc_bridge_abi_version", "bridge LayerNorm"),
                SideHeader("SURFACE", "transception_surface.h", "TC_SURFACE_ABI_VERSION", "tc_surface_abi_version", "surface metrics"),
                SideHeader("UNCERT", "transception_uncertainty.h", "TC_UNCERT_ABI_VERSION", "tc_uncert_abi_version", "uncertainty / calibration"),
                SideHeader("TOPK", "transception_topk.h", "TC_TOPK_ABI_VERSION", "tc_topk_abi_version", "top-k loss"),
                SideHeader("LOSS", "transception_loss.h", "TC_LOSS_ABI_VERSION", "tc_loss_abi_version", "focal / Tversky loss"))

SCALARS = {"int": C.c_int, "long long": C.c_longlong, "float": C.c_float, "double": C.c_double,
           "unsigned": C.c_uint, "unsigned int": C.c_uint}
POINTEES = set(SCALARS) | {"void", "unsigned char"}       # what a pointer may point to, besides the structs; every pointer is a c_void_p


class HeaderError(ValueError):
    pass


class Function(NamedTuple):
    restype: type
    argtypes: list
    query: bool               # marked TC_QUERY: returns a value; otherwise an int status that the binding checks


class Header(NamedTuple):
    functions: dict           # name -> Function, in declaration order
    structs: dict             # name -> ctypes.Structure subclass
    constants: dict           # enum members and #define TC_* values


_TOKEN = re.compile(r"\s*(\d+|<<|[()|+-])")
_LEVELS = ({"|": operator.or_}, {"<<": operator.lshift}, {"+": operator.add, "-": operator.sub})    # loosest first, as in C


def evaluate(expr: str) -> int:
    """An integer constant expression of decimal integers, parentheses, <<, |, + and - (nothing else: no names, no calls)."""
    toks, pos, expr = [], 0, expr.strip()
    while pos < len(expr):
        m = _TOKEN.match(expr, pos)
        if not m:
            raise HeaderError(f"constant expression {expr!r}: cannot read {expr[pos:]!r}")
        toks.append(m.group(1))
        pos = m.end()
    toks.reverse()                                        # consumed from the end

    def level(i):
        if i == len(_LEVELS):
            t = toks.pop() if toks else ""
            if t in ("-", "+"):
                return level(i) if t == "+" else -level(i)
            if t == "(":
                v = level(0)
                if not toks or toks.pop() != ")":
                    raise HeaderError(f"constant expression {expr!r}: missing )")
                return v
            if t.isdigit():
                return int(t)
            raise HeaderError(f"constant expression {expr!r}: operand expected")
        v = level(i + 1)
        while toks and toks[-1] in _LEVELS[i]:
            v = _LEVELS[i][toks.pop()](v, level(i + 1))
        return v

    v = level(0)
    if toks:
        raise HeaderError(f"constant expression {expr!r}: unexpected {toks[-1]!r}")
    return v


_DECLARATOR = re.compile(r"\s*([A-Za-z_][\w\s]*?(?:\s|\*))\s*(\w+)\s*(?:\[(\d+)\])?\s*")


def _pointers(pointee: str) -> dict:
    return {pointee + "*": C.c_void_p, "const " + pointee + "*": C.c_void_p}


def _ctype(decl: str, known: dict, where: str):
    """'const float* x' -> ('x', c_void_p); 'double m[6]' -> ('m', c_double * 6).  known: type text -> ctypes type."""
    m = _DECLARATOR.fullmatch(decl)
    t = m and known.get(" ".join(m.group(1).split()).replace(" *", "*"))
    if t is None:
        raise HeaderError(f"{where}: unknown type in {decl.strip()!r}")
    return m.group(2), t * int(m.group(3)) if m.group(3) else t


def _fields(body: str, known: dict, where: str) -> list:
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *more = decl.split(",")                    # 'int M, N, K': the declarators after the first repeat its type
        name, t = _ctype(first, known, where)
        if more and "*" in first:
            raise HeaderError(f"{where}: several declarators of a pointer type in {decl!r}")
        fields.append((name, t))
        for d in more:
            fields.append(_ctype(first[:first.rindex(name)] + d, known, where))
    return fields


_ITEM = re.compile(r"""\s*(?:
      (?P<wrap>extern\s*"C"\s*\{ | \})
    | enum\s*\{(?P<enum>[^{};]*)\}\s*;
    | typedef\s+struct\s*(?P<tag>\w*)\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | (?P<query>TC_QUERY\s+)?(?P<ret>[A-Za-z_][\w ]*?)\s+(?P<fn>tc_\w+)\s*\((?P<args>[^(){};]*)\)\s*;
    )""", re.X)


def parse(text: str) -> Header:
    functions, structs, constants = {}, {}, {}
    known = dict(SCALARS)                                 # type text -> ctypes type; the structs' pointers join as they are declared
    for pointee in POINTEES:
        known.update(_pointers(pointee))
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)

    def directive(m):                                     # conditionals are dropped, not evaluated: both the C and the C++ reading
        word, rest = m.group(1), m.group(2).split(None, 1)      # of the header declare the same ABI
        if word == "define" and rest and rest[0].startswith("TC_"):
            if len(rest) == 2:
                constants[rest[0]] = evaluate(rest[1])
            elif rest[0] != "TC_QUERY":
                raise HeaderError(f"#define {rest[0]}: a marker this parser does not know")
        elif word not in ("ifndef", "ifdef", "endif") and not (word == "define" and len(rest) == 1):
            raise HeaderError(f"preprocessor line {m.group(0).strip()!r} is not understood")
        return ""

    text = re.sub(r"^[ \t]*#[ \t]*(\w*)(.*)$", directive, text, flags=re.M)
    pos, depth, end = 0, 0, len(text.rstrip())
    while pos < end:
        m = _ITEM.match(text, pos)
        if not m:
            raise HeaderError(f"cannot parse the header at {text[pos:].strip()[:80]!r}")
        pos = m.end()
        if m.group("wrap"):
            depth += 1 if m.group("wrap") != "}" else -1
            if depth not in (0, 1):
                raise HeaderError('unbalanced extern "C" wrapper')
        elif m.group("enum") is not None:
            for member in filter(None, (e.strip() for e in m.group("enum").split(","))):
                name, eq, value = member.partition("=")
                if not eq or not re.fullmatch(r"TC_\w+", name.strip()):
                    raise HeaderError(f"enum member {member!r} is not NAME = value")
                constants[name.strip()] = evaluate(value)
        elif m.group("struct"):
            name = m.group("struct")
            if m.group("tag") not in ("", name) or name in structs:
                raise HeaderError(f"struct {name}: tag {m.group('tag')!r} or a second definition")
            structs[name] = type(name, (C.Structure,), {"_fields_": _fields(m.group("body"), known, f"struct {name}")})
            known.update(_pointers(name))
        else:
            name, ret, args = m.group("fn"), " ".join(m.group("ret").split()), m.group("args").strip()
            if ret not in SCALARS or name in functions:
                raise HeaderError(f"{name}: unknown return type {ret!r} or a second declaration")
            if not m.group("query") and ret != "int":
                raise HeaderError(f"{name} returns {ret}, not a status: mark it TC_QUERY")
            argtypes = [] if args in ("", "void") else [_ctype(a, known, name)[1] for a in args.split(",")]
            functions[name] = Function(SCALARS[ret], argtypes, bool(m.group("query")))
    if depth:
        raise HeaderError('unbalanced extern "C" wrapper')
    return Header(functions, structs, constants)


def load(path: str = HEADER) -> Header:
    with open(path) as f:
        return parse(f.read())
