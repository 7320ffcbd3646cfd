"""ctypes binding of libccd_hip.so (the C ABI of include/ccd_hip.h).

There is NO CPU fallback: if the shared library is missing or a call fails, a RuntimeError is raised.
The library is built in-tree by `__graft_entry__.build()` / `ccd_amd/csrc/build.sh` as ccd_amd/libccd_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CCD_HIP_LIB") or os.path.join(_HERE, "libccd_hip.so")   # override: lab builds (tools/gemm_lab.py)

_handle = None            # ctypes.CDLL once loaded
_stream_override = None   # tests of the ABI may pin the stream argument

HEADER_PATH = os.path.join(_HERE, "..", "include", "ccd_hip.h")

_SCALARS = {"int": C.c_int, "long": C.c_long, "float": C.c_float, "double": C.c_double, "uint64_t": C.c_uint64, "const char*": C.c_char_p}
_RETURNS = {"int": C.c_int, "long": C.c_long, "const char*": C.c_char_p}
# element type of a pointer parameter -> the tensor dtypes it takes (None: untyped, any dtype)
_ELEMENT_DTYPES = {"float": (torch.float32,), "ccd_bf16": (torch.bfloat16,), "uint16_t": (torch.float16,), "double": (torch.float64,),
                   "int": (torch.int32,), "long": (torch.int64,), "int64_t": (torch.int64,), "uint64_t": (torch.int64, torch.uint64),
                   "uint8_t": (torch.uint8,), "void": None}


def _pointer_type(elem, dtypes):
    """The argtype of an `elem*` parameter.  It takes None (NULL), an int (a raw address), a ctypes array / structure / pointer, or a
    tensor: its data_ptr(), provided the dtype is the header's and the innermost dimension is dense."""
    want = " or ".join(str(d)[6:] for d in dtypes) if dtypes else ""

    def from_param(cls, v):
        if isinstance(v, torch.Tensor):
            if dtypes is not None and v.dtype not in dtypes:
                raise TypeError(f"expects {want}, got {str(v.dtype)[6:]}")
            if not v.is_contiguous() and v.stride(-1) != 1 and v.shape[-1] > 1:      # (one call for the usual, dense tensor)
                raise ValueError("innermost dimension must be contiguous")
            return C.c_void_p(v.data_ptr())
        if v is None:
            return None
        return C.byref(v) if isinstance(v, C.Structure) else C.c_void_p.from_param(v)

    return type(f"{elem}_p", (), {"elem": elem, "dtypes": dtypes, "from_param": classmethod(from_param)})


def parse_header(text):
    """name -> (restype, [(argtype, parameter name)]) of every ccd_* prototype of include/ccd_hip.h.  Anything the tables above do not
    know is an error here, at import: a guessed argument type would corrupt a stride or a pointer on the device."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$|extern\s+\"C\"\s*\{", " ", text, flags=re.M)
    pointers = dict(_ELEMENT_DTYPES)
    for name in re.findall(r"typedef\s+struct[^{;]*\{[^}]*\}\s*(\w+)\s*;", text):
        pointers[name] = None                                    # descriptor structs: host or device memory, no dtype
    text = re.sub(r"typedef\s+struct[^{;]*\{[^}]*\}\s*\w+\s*;|typedef[^;{]*;", " ", text)
    pointers = {elem + "*": _pointer_type(elem, dtypes) for elem, dtypes in pointers.items()}

    def ctype(decl, table, where):
        decl = re.sub(r"\s*\*", "*", " ".join(decl.split()))
        if decl not in table and decl.removeprefix("const ") not in table:
            raise ImportError(f"ccd_amd: include/ccd_hip.h: no ctypes mapping for '{decl}' in {where}")
        return table[decl] if decl in table else table[decl.removeprefix("const ")]

    protos = {}
    for stmt in text.replace("}", " ").split(";"):               # (the brace that closes extern "C")
        if not stmt.strip():
            continue
        m = re.fullmatch(r"\s*([\w\s\*]+?)\s*\b(ccd_\w+)\s*\(([^()]*)\)\s*", stmt)
        if m is None:
            raise ImportError(f"ccd_amd: include/ccd_hip.h: cannot parse '{' '.join(stmt.split())}'")
        ret, name, params = m.groups()
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            decl, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", p, flags=re.S).groups()
            args.append((ctype(decl, {**_SCALARS, **pointers}, f"{name}({pname})"), pname))
        protos[name] = (ctype(ret, _RETURNS, name), args)
    return protos


with open(HEADER_PATH) as _f:
    PROTOTYPES = parse_header(_f.read())
SIGNATURES = {name: [t for t, _ in args] for name, (_, args) in PROTOTYPES.items()}       # name -> argtypes


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach argtypes/restypes; raises AttributeError if the library lacks a declared symbol."""
    for name, (restype, _) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = SIGNATURES[name]
        fn.restype = restype
    return lib


def argument_error(name, err):
    """ctypes.ArgumentError of a call of `name` -> the TypeError / ValueError a pointer type raised, naming the header's parameter."""
    m = re.fullmatch(r"argument (\d+): (\w+): (.*)", str(err), flags=re.S)
    kind = {"TypeError": TypeError, "ValueError": ValueError}.get(m.group(2)) if m else None
    if kind is None:
        return err
    return kind(f"{name}: {PROTOTYPES[name][1][int(m.group(1)) - 1][1]} {m.group(3)}")


def get() -> C.CDLL:
    global _handle
    if _handle is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"ccd_amd: HIP library not found at {LIB_PATH}. Build it with `python -c 'import __graft_entry__ as g; "
                "g.build()'` (hipcc --offload-arch=gfx950). ccd_amd has no CPU fallback.")
        _handle = bind(C.CDLL(LIB_PATH))
    return _handle


def stream() -> int:
    if _stream_override is not None:
        return _stream_override
    return torch.cuda.current_stream().cuda_stream


def check(code: int, what: str):
    if code != 0:
        kind = {-1: "invalid argument", -2: "unsupported shape"}.get(code, f"hipError {code}")
        raise RuntimeError(f"ccd_amd: {what} failed: {kind}")


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()
