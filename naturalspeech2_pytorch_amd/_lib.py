"""ctypes binding of libns2hip.so, derived from its C ABI: include/ns2hip.h (and include/ns2hip_optim.h, the optimizer step, and
include/ns2hip_pitch.h, the pitch extractor, include/ns2hip_ragged.h, ragged batches, include/ns2hip_ragged_front.h, ragged prompts
and text, include/ns2hip_ragged_train.h, ragged training batches, include/ns2hip_head_dim_train.h, training at head dims 32 and 128, and
include/ns2hip_ragged_audio.h, ragged raw audio, include/ns2hip_fold.h, the feed-forward fold, and include/ns2hip_ragged_cond_train.h,
ragged text and prompts in training, include/ns2hip_ragged_skip.h, skipping in a ragged sampling batch, and
include/ns2hip_ragged_skip_train.h, skipping in a ragged training batch, and include/ns2hip_tail_fold.h, the Wavenet tail fold and the
wide RMSNorm kernel, each into tables of its own) is parsed once, at import.

The HIP library is the product: importing this module FAILS LOUDLY when the header or the shared object is missing or the
library does not export the full ABI -- there is no CPU / PyTorch fallback for the hot path.

The header is the one owner of the ABI.  Its `#define NS2_<NAME> <int>` lines become the status constants, every
`typedef struct { ... } name;` a ctypes.Structure, every `ret ns2_name(args);` a row of SIGNATURES.  A new entry point needs
its declaration there and nothing here.  One mapping rule, and nothing is guessed (what it does not cover raises Ns2Error
naming the declaration):
    int -> c_int;  unsigned, unsigned int -> c_uint;  uint32_t -> c_uint32;  int64_t -> c_int64;  float -> c_float;
    double -> c_double;  a void return -> None;  const char* -> c_char_p;
    a pointer to a struct whose body the header gives -> POINTER(that class);  a pointer to a pointer -> POINTER(c_void_p);
    every other pointer (to a scalar, to void, to the opaque ns2_model / ns2_weight) -> c_void_p;
    a struct field that is a pointer -> c_void_p.
The header cannot say whether an `int*` is a host out-parameter or device memory (most are device pointers, passed as
integers), so host out-parameters are c_void_p too: byref(), a ctypes array and None all pass, but ctypes no longer checks
their element type.  That is the accepted price of having no second, hand-kept table.
"""
import ctypes
import os
import re
from ctypes import c_char_p, c_void_p, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NS2_LIB", os.path.join(_HERE, "libns2hip.so"))   # NS2_LIB: experiment builds (tools/)
HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip.h")
OPTIM_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_optim.h")   # the optimizer step: a header and tables of its own
PITCH_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_pitch.h")   # the pitch extractor: likewise
RAGGED_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged.h")   # per-utterance lengths: likewise
FRONT_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_front.h")   # ... through the front-end: likewise
RAGGED_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_train.h")   # ... in the training pass: likewise
HEAD_DIM_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_head_dim_train.h")   # training at head dims 32 / 128: likewise
RAGGED_AUDIO_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_audio.h")   # lengths in mel, pitch and the RVQ term: likewise
FOLD_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_fold.h")   # the feed-forward fold: likewise
RAGGED_COND_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_cond_train.h")   # lengths through the conditioning's training pass: likewise
RAGGED_SKIP_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_skip.h")   # skipping the hidden row tiles of a ragged sampling batch: likewise
RAGGED_SKIP_TRAIN_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_ragged_skip_train.h")   # ... of a ragged training batch: likewise
TAIL_FOLD_HEADER_PATH = os.path.join(_HERE, "..", "include", "ns2hip_tail_fold.h")   # the Wavenet tail fold, the wide RMSNorm kernel: likewise


class Ns2Error(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "unsigned int": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
            "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}


def _ctype(ctype, structs, decl, field=False):
    """the ctypes type of the C type `ctype` (declarator name removed) by the module's rule; an Ns2Error naming `decl` if it has none"""
    stars = ctype.count("*")
    base = " ".join(w for w in ctype.replace("*", " ").split() if w != "const")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars not in (1, 2) or not re.fullmatch(r"\w+( \w+)?", base):
        raise Ns2Error(f"include/ns2hip.h: no ctypes mapping for `{ctype.strip()}` in `{decl}`")
    if field:
        return c_void_p
    if stars == 2:
        return POINTER(c_void_p)
    if base == "char" and "const" in ctype.split():
        return c_char_p
    return POINTER(structs[base]) if base in structs else c_void_p


def _declarator(text, decl):
    """`type name` -> (type, name)"""
    m = re.fullmatch(r"([\w\s*]*[\s*])(\w+)", text.strip())
    if not m:
        raise Ns2Error(f"include/ns2hip.h: cannot read `{text.strip()}` in `{decl}`")
    return m.group(1), m.group(2)


def parse_header(text):
    """(constants, structs, signatures) of a header text: {NS2_NAME: int}, {typedef name: ctypes.Structure subclass},
    {ns2_name: (restype, argtypes)}.  Plain `re`, no C front end; every statement is one of the three forms or an Ns2Error."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    consts = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NS2_\w+)[ \t]+(.*?)[ \t]*$", text, flags=re.M):
        if not re.fullmatch(r"-?\d+", value):
            raise Ns2Error(f"include/ns2hip.h: `#define {name} {value}` is not an integer")
        consts[name] = int(value)
    text = re.sub(r"^[ \t]*#ifdef __cplusplus\n.*?\n[ \t]*#endif[^\n]*$", " ", text, flags=re.S | re.M)   # extern "C" { / }
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    structs = {}

    def struct(m):
        name, fields = m.group(2), []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(1).split(";"))):
            first, *more = decl.split(",")                      # `int ldq, q_col0;`: the type belongs to every declarator
            ctype, field = _declarator(first, f"{name}: {decl}")
            if more and ("*" in decl or not all(f.strip().isidentifier() for f in more)):
                raise Ns2Error(f"include/ns2hip.h: cannot read `{decl}` in `{name}`")
            ct = _ctype(ctype, structs, f"{name}: {decl}", field=True)
            fields += [(f.strip(), ct) for f in [field] + more]
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields, "__doc__": f"{name} (include/ns2hip.h)"})
        return " "
    text = re.sub(r"\btypedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    sigs = {}
    for decl in filter(None, (" ".join(d.split()) for d in text.split(";"))):
        if re.fullmatch(r"typedef struct (\w+) \1", decl):       # an opaque handle: its pointers are c_void_p
            continue
        m = re.fullmatch(r"([\w\s*]+?)\b(ns2_\w+) ?\(([^()]*)\)", decl)
        if not m:
            raise Ns2Error(f"include/ns2hip.h: cannot read `{decl}`")
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        args = [] if args == "void" else [_ctype(_declarator(a, decl)[0], structs, decl) for a in args.split(",")]
        sigs[name] = (None if ret == "void" else _ctype(ret, structs, decl), args)
    return consts, structs, sigs


if not os.path.exists(HEADER_PATH):
    raise Ns2Error(f"{HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(HEADER_PATH) as _f:
    CONSTANTS, STRUCTS, SIGNATURES = parse_header(_f.read())     # SIGNATURES: name -> (restype, argtypes)
NS2_OK, NS2_ERR_ARG, NS2_ERR_HIP, NS2_ERR_STATE, NS2_UNAVAILABLE = (
    CONSTANTS[k] for k in ("NS2_OK", "NS2_ERR_ARG", "NS2_ERR_HIP", "NS2_ERR_STATE", "NS2_UNAVAILABLE"))
ModelConfig, LinearArgs, AttnArgs, AttnBwdArgs, RepackPart = (
    STRUCTS[k] for k in ("ns2_model_config", "ns2_linear_args", "ns2_attn_args", "ns2_attn_bwd_args", "ns2_repack_part"))

if not os.path.exists(OPTIM_HEADER_PATH):
    raise Ns2Error(f"{OPTIM_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(OPTIM_HEADER_PATH) as _f:                              # same rule, tables of its own: SIGNATURES / STRUCTS / header_symbols()
    OPTIM_CONSTANTS, OPTIM_STRUCTS, OPTIM_SIGNATURES = parse_header(_f.read())      # keep describing ns2hip.h alone
OptimTensor, OptimConfig = (OPTIM_STRUCTS[k] for k in ("ns2_optim_tensor", "ns2_optim_config"))

if not os.path.exists(PITCH_HEADER_PATH):
    raise Ns2Error(f"{PITCH_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(PITCH_HEADER_PATH) as _f:
    _, _, PITCH_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_HEADER_PATH) as _f:                             # ns2_attn_args / ns2_model are ns2hip.h's (its #include is not followed): their
    _, _, RAGGED_SIGNATURES = parse_header(_f.read())            # pointers are c_void_p here -- pass ctypes.byref(block)

if not os.path.exists(FRONT_HEADER_PATH):
    raise Ns2Error(f"{FRONT_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(FRONT_HEADER_PATH) as _f:
    _, _, FRONT_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_TRAIN_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_TRAIN_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_TRAIN_HEADER_PATH) as _f:                       # (ns2_attn_args / ns2_attn_bwd_args: c_void_p here, as in RAGGED_SIGNATURES)
    _, _, RAGGED_TRAIN_SIGNATURES = parse_header(_f.read())

if not os.path.exists(HEAD_DIM_TRAIN_HEADER_PATH):
    raise Ns2Error(f"{HEAD_DIM_TRAIN_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(HEAD_DIM_TRAIN_HEADER_PATH) as _f:                     # (the argument blocks: c_void_p here too)
    _, _, HEAD_DIM_TRAIN_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_AUDIO_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_AUDIO_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_AUDIO_HEADER_PATH) as _f:
    _, _, RAGGED_AUDIO_SIGNATURES = parse_header(_f.read())

if not os.path.exists(FOLD_HEADER_PATH):
    raise Ns2Error(f"{FOLD_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(FOLD_HEADER_PATH) as _f:
    _, _, FOLD_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_COND_TRAIN_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_COND_TRAIN_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_COND_TRAIN_HEADER_PATH) as _f:
    _, _, RAGGED_COND_TRAIN_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_SKIP_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_SKIP_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_SKIP_HEADER_PATH) as _f:                        # (the argument blocks, ns2_weight and ns2_model_config: c_void_p here too)
    _, _, RAGGED_SKIP_SIGNATURES = parse_header(_f.read())

if not os.path.exists(RAGGED_SKIP_TRAIN_HEADER_PATH):
    raise Ns2Error(f"{RAGGED_SKIP_TRAIN_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(RAGGED_SKIP_TRAIN_HEADER_PATH) as _f:                  # (ns2_linear_args: c_void_p here too -- pass ctypes.byref(block))
    _, _, RAGGED_SKIP_TRAIN_SIGNATURES = parse_header(_f.read())

if not os.path.exists(TAIL_FOLD_HEADER_PATH):
    raise Ns2Error(f"{TAIL_FOLD_HEADER_PATH} not found: the binding is derived from the header, it ships with the package's source tree")
with open(TAIL_FOLD_HEADER_PATH) as _f:
    _, _, TAIL_FOLD_SIGNATURES = parse_header(_f.read())

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
    for name, (res, args) in {**SIGNATURES, **OPTIM_SIGNATURES, **PITCH_SIGNATURES, **RAGGED_SIGNATURES, **FRONT_SIGNATURES,
                              **RAGGED_TRAIN_SIGNATURES, **HEAD_DIM_TRAIN_SIGNATURES, **RAGGED_AUDIO_SIGNATURES, **FOLD_SIGNATURES,
                              **RAGGED_COND_TRAIN_SIGNATURES, **RAGGED_SKIP_SIGNATURES, **RAGGED_SKIP_TRAIN_SIGNATURES,
                              **TAIL_FOLD_SIGNATURES}.items():
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


def header_symbols():
    """Symbols declared in include/ns2hip.h (used by the CPU test that the .so exports the whole ABI)."""
    return sorted(SIGNATURES)


def optim_header_symbols():
    """Symbols declared in include/ns2hip_optim.h"""
    return sorted(OPTIM_SIGNATURES)


def pitch_header_symbols():
    """Symbols declared in include/ns2hip_pitch.h"""
    return sorted(PITCH_SIGNATURES)


def ragged_header_symbols():
    """Symbols declared in include/ns2hip_ragged.h"""
    return sorted(RAGGED_SIGNATURES)


def front_header_symbols():
    """Symbols declared in include/ns2hip_ragged_front.h"""
    return sorted(FRONT_SIGNATURES)


def ragged_train_header_symbols():
    """Symbols declared in include/ns2hip_ragged_train.h"""
    return sorted(RAGGED_TRAIN_SIGNATURES)


def head_dim_train_header_symbols():
    """Symbols declared in include/ns2hip_head_dim_train.h"""
    return sorted(HEAD_DIM_TRAIN_SIGNATURES)


def ragged_audio_header_symbols():
    """Symbols declared in include/ns2hip_ragged_audio.h"""
    return sorted(RAGGED_AUDIO_SIGNATURES)


def fold_header_symbols():
    """Symbols declared in include/ns2hip_fold.h"""
    return sorted(FOLD_SIGNATURES)


def ragged_cond_train_header_symbols():
    """Symbols declared in include/ns2hip_ragged_cond_train.h"""
    return sorted(RAGGED_COND_TRAIN_SIGNATURES)


def ragged_skip_header_symbols():
    """Symbols declared in include/ns2hip_ragged_skip.h"""
    return sorted(RAGGED_SKIP_SIGNATURES)


def ragged_skip_train_header_symbols():
    """Symbols declared in include/ns2hip_ragged_skip_train.h"""
    return sorted(RAGGED_SKIP_TRAIN_SIGNATURES)


def tail_fold_header_symbols():
    """Symbols declared in include/ns2hip_tail_fold.h"""
    return sorted(TAIL_FOLD_SIGNATURES)
