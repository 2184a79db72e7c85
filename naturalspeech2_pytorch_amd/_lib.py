"""ctypes binding of libns2hip.so, derived from its C ABI: the headers under include/ that HEADERS lists, parsed once, at import, in
that order.

The HIP library is the product: importing this module FAILS LOUDLY when a header or the shared object is missing or the
library does not export the full ABI -- there is no CPU / PyTorch fallback for the hot path.

The headers are the one owner of the ABI.  A header's `#define NS2_<NAME> <int>` lines become constants, every
`typedef struct { ... } name;` a ctypes.Structure, every `ret ns2_name(args);` a row of SIGNATURES; ABI keeps the three tables of
each header, CONSTANTS / STRUCTS / SIGNATURES are their unions, and no name may be declared twice.  A new entry point needs its
declaration in the header of its concern, behind the entry it varies, and nothing here.  One mapping rule, and nothing is guessed (what it
does not cover raises Ns2Error naming the file and the declaration):
    int -> c_int;  unsigned, unsigned int -> c_uint;  uint32_t -> c_uint32;  int64_t -> c_int64;  float -> c_float;
    double -> c_double;  a void return -> None;  const char* -> c_char_p;
    a pointer to a struct whose body this header or one before it in HEADERS gives -> POINTER(that class);
    a pointer to a pointer -> POINTER(c_void_p);
    every other pointer (to a scalar, to void, to the opaque ns2_model / ns2_weight) -> c_void_p;
    a struct field that is a pointer -> c_void_p.
A header cannot say whether an `int*` is a host out-parameter or device memory (most are device pointers, passed as
integers), so host out-parameters are c_void_p too: byref(), a ctypes array and None all pass, but ctypes no longer checks
their element type.  That is the accepted price of having no second, hand-kept table.
"""
import collections
import ctypes
import os
import re
from ctypes import c_char_p, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NS2_LIB", os.path.join(_HERE, "libns2hip.so"))   # NS2_LIB: experiment builds (tools/)
INCLUDE_DIR = os.path.join(_HERE, "..", "include")
HEADERS = (
    "ns2hip.h",             # the core that sampling needs; first: the others use its structs and status codes
    "ns2hip_frontend.h",    # the conditioning front-end: DurationPitchPredictor, Aligner, ragged prompts and text
    "ns2hip_audio.h",       # raw audio and the codec: mel, pitch, resampling, SEANet / LSTM pieces, RVQ
    "ns2hip_train.h",       # the training pass
    "ns2hip_optim.h",       # the optimizer step
)


class Ns2Error(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
            "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(ctype, structs, decl, where, field=False):
    """the ctypes type of the C type `ctype` (declarator name removed) by the module's rule; an Ns2Error naming `decl` if it has none"""
    stars = ctype.count("*")
    base = " ".join(w for w in ctype.replace("*", " ").split() if w != "const")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars not in (1, 2) or not re.fullmatch(r"\w+( \w+)?", base):
        raise Ns2Error(f"{where}: no ctypes mapping for `{ctype.strip()}` in `{decl}`")
    if field:
        return c_void_p
    if stars == 2:
        return POINTER(c_void_p)
    if base == "char" and "const" in ctype.split():
        return c_char_p
    return POINTER(structs[base]) if base in structs else c_void_p


def _declarator(text, decl, where):
    """`type name` -> (type, name)"""
    m = re.fullmatch(r"([\w\s*]*[\s*])(\w+)", text.strip())
    if not m:
        raise Ns2Error(f"{where}: cannot read `{text.strip()}` in `{decl}`")
    return m.group(1), m.group(2)


def parse_header(text, structs=None, where="include/ns2hip.h"):
    """(constants, structs, signatures) of a header text: {NS2_NAME: int}, {typedef name: ctypes.Structure subclass},
    {ns2_name: (restype, argtypes)}.  Plain `re`, no C front end; every statement is one of the three forms or an Ns2Error, which
    names the file `where`.  `structs` holds the structs of the headers read before: a pointer to one is typed, defining one again
    is an error, and the returned dict holds this header's own."""
    known, structs = dict(structs or {}), {}                    # every struct a pointer may name; this header's own
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NS2_\w+)[ \t]+(.*?)[ \t]*$", text, flags=re.M):
        if not re.fullmatch(r"-?\d+", value):
            raise Ns2Error(f"{where}: `#define {name} {value}` is not an integer")
        consts[name] = int(value)
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?\n[ \t]*#endif[^\n]*$", " ", text, flags=re.S | re.M)   # extern "C" { / }
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)

    def struct(m):
        name, fields = m.group(2), []
        if name in known:
            raise Ns2Error(f"{where}: `typedef struct {{...}} {name};` is already defined: {known[name].__doc__}")
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            first, *more = decl.split(",")                      # `int ldq, q_col0;`: the type belongs to every declarator
            ctype, field = _declarator(first, f"{name}: {decl}", where)
            if more and ("*" in decl or not all(f.strip().isidentifier() for f in more)):
                raise Ns2Error(f"{where}: cannot read `{decl}` in `{name}`")
            ct = _ctype(ctype, known, f"{name}: {decl}", where, field=True)
            fields += [(f.strip(), ct) for f in [field] + more]
        structs[name] = known[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} ({where})"})
        return " "
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    sigs = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        if re.fullmatch(r"typedef struct (\w+) \1", decl):       # an opaque handle: its pointers are c_void_p
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(ns2_\w+) ?\(([^()]*)\)", decl)
        if not m:
            raise Ns2Error(f"{where}: cannot read `{decl}`")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        args = [] if args == "void" else [_ctype(_declarator(a, decl, where)[0], known, decl, where) for a in args.split(",")]
        sigs[name] = (None if ret == "void" else _ctype(ret, known, decl, where), args)
    return consts, structs, sigs


Header = collections.namedtuple("Header", "constants structs signatures")


def load_abi(include_dir, headers):
    """{header file name: Header(constants, structs, signatures)} of the `headers` under `include_dir`, parsed in that order, each with
    the structs of those before it; an Ns2Error if a file is missing or a name is declared in two of them"""
    abi, owner, structs = {}, {}, {}
    for name in headers:
        path = os.path.join(include_dir, name)
        where = os.path.join(os.path.basename(os.path.normpath(include_dir)), name)
        if not os.path.exists(path):
            raise Ns2Error(f"{path} not found: the binding is derived from the header, it ships with the package's source tree")
        with open(path) as f:
            abi[name] = Header(*parse_header(f.read(), structs, where))
        for sym in (*abi[name].constants, *abi[name].signatures):    # (a struct defined twice: parse_header has refused it)
            if sym in owner:
                raise Ns2Error(f"{where}: `{sym}` is already declared in {owner[sym]}")
            owner[sym] = where
        structs.update(abi[name].structs)
    return abi


ABI = load_abi(INCLUDE_DIR, HEADERS)
CONSTANTS, STRUCTS, SIGNATURES = (                               # the unions over all headers; SIGNATURES: name -> (restype, argtypes)
    {k: v for h in ABI.values() for k, v in h[i].items()} for i in range(3))
NS2_OK, NS2_ERR_ARG, NS2_ERR_HIP, NS2_ERR_STATE, NS2_UNAVAILABLE = (
    CONSTANTS[k] for k in ("NS2_OK", "NS2_ERR_ARG", "NS2_ERR_HIP", "NS2_ERR_STATE", "NS2_UNAVAILABLE"))
ModelConfig, LinearArgs, AttnArgs, AttnBwdArgs, RepackPart, OptimTensor, OptimConfig = (
    STRUCTS[k] for k in ("ns2_model_config", "ns2_linear_args", "ns2_attn_args", "ns2_attn_bwd_args", "ns2_repack_part",
                         "ns2_optim_tensor", "ns2_optim_config"))

_lib = None


def load():
    """Load libns2hip.so and bind every symbol of the ABI; raises Ns2Error if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise Ns2Error(f"{LIB_PATH} not found: build it with `python __graft_entry__.py` "
                       f"(or naturalspeech2_pytorch_amd/csrc/build.sh); there is no fallback path")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise Ns2Error(f"libns2hip.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().ns2_last_error()
        raise Ns2Error(f"{what} failed (rc={rc}): {msg.decode() if msg else '?'}")


def header_symbols(header=None):
    """The sorted entry points that `header` (a name in HEADERS) declares; of the whole ABI when it is None."""
    return sorted(SIGNATURES if header is None else ABI[header].signatures)
