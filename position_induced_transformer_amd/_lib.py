"""ctypes binding of csrc/libpit_hip.so, derived from the C ABI's own declaration, include/pit_hip.h.

The header is parsed once, at import: prototypes -> PROTOTYPES / SIGNATURES / LONG_RETURN, structs -> the _fields_ of the
ctypes.Structure classes, object-like integer #defines -> DEFINES.  Nothing of it is restated here, so an ABI addition touches
the header (and ADDED_LATER, when it joins a released version) and nothing else on the Python side.

There is no fallback: if the library is missing or a symbol is absent this raises, and
every op in this package goes through it.  torch is imported first so that the HIP
runtime already loaded by PyTorch-ROCm is the one the library binds to."""
from __future__ import annotations

import collections
import ctypes
import operator
import os
import re
import types

import torch  # noqa: F401  (must precede the CDLL load)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PIT_LIB_PATH") or os.path.join(_HERE, "csrc", "libpit_hip.so")   # (override: diagnostic builds, tools/)
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "pit_hip.h"))

# ---- the header's text -> prototypes, structs, constants ------------------------------------------------------------------------
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "float": ctypes.c_float,
            "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "long": ctypes.c_long, "const char*": ctypes.c_char_p}
_BINARY = {"|": (1, operator.or_), "&": (2, operator.and_), "<<": (3, operator.lshift), ">>": (3, operator.rshift),
           "+": (4, operator.add), "-": (4, operator.sub), "*": (5, operator.mul)}          # C's precedence
_TOKEN = re.compile(r"0[xX][0-9a-fA-F]+[uUlL]*|\d+[uUlL]*|PIT_\w+|<<|>>|[-+*|&()]")

Prototype = collections.namedtuple("Prototype", "restype argtypes argnames")
Header = collections.namedtuple("Header", "prototypes structs defines")


def _ctype(c_type: str, where: str):
    """The ctypes type of a parameter or field: any pointer is c_void_p, a scalar must be in the map (never a default)."""
    if "*" in c_type:
        return ctypes.c_void_p
    c_type = " ".join(w for w in c_type.split() if w not in ("const", "struct"))
    if c_type not in _SCALARS:
        raise ValueError(f"{where}: no ctypes type for the C type {c_type!r}")
    return _SCALARS[c_type]


def _declarators(text: str, where: str) -> list:
    """[(name, ctypes type), ...] of one C declaration: `const float* x`, `double* const* p`, `int a, b`, `float *e, *q`."""
    out, base = [], None
    for piece in text.split(","):
        m = re.fullmatch(r"\s*(.*?)(\w+)\s*", piece, flags=re.S)
        if not m:
            raise ValueError(f"{where}: cannot parse the declaration {' '.join(text.split())!r}")
        spec, name = m.groups()
        if base is None:                      # the first declarator names the base type; the `*`s belong to each declarator
            base, star, rest = spec.partition("*")
            spec = star + rest
        elif spec.replace("*", " ").replace("const", " ").strip():
            raise ValueError(f"{where}: cannot parse the declaration {' '.join(text.split())!r}")
        out.append((name, _ctype(base + spec, f"{where}, {name}")))
    return out


def _evaluate(expr: str, known: dict, name: str) -> int:
    """An integer #define's value: digits (L / U suffixes dropped), + - * << >> | & ( ) and earlier PIT_ names - nothing else."""
    toks = _TOKEN.findall(expr)
    if "".join(toks) != "".join(expr.split()) or not toks:
        raise ValueError(f"#define {name}: {expr.strip()!r} is not an integer expression this binding evaluates")
    pos = 0

    def take():
        nonlocal pos
        if pos >= len(toks):
            raise ValueError(f"#define {name}: {expr.strip()!r} ends early")
        pos += 1
        return toks[pos - 1]

    def atom() -> int:
        t = take()
        if t == "(":
            v = binary(1)
            if take() != ")":
                raise ValueError(f"#define {name}: unbalanced parentheses in {expr.strip()!r}")
            return v
        if t in "+-":
            return atom() if t == "+" else -atom()
        if t.startswith("PIT_"):
            if t not in known:
                raise ValueError(f"#define {name}: refers to {t}, which no earlier #define gives a value")
            return known[t]
        if t[0].isdigit():
            return int(t.rstrip("uUlL"), 0)
        raise ValueError(f"#define {name}: unexpected {t!r} in {expr.strip()!r}")

    def binary(min_prec: int) -> int:
        v = atom()
        while pos < len(toks) and toks[pos] in _BINARY and _BINARY[toks[pos]][0] >= min_prec:
            prec, fn = _BINARY[take()]
            v = fn(v, binary(prec + 1))
        return v

    value = binary(1)
    if pos != len(toks):
        raise ValueError(f"#define {name}: unexpected {toks[pos]!r} in {expr.strip()!r}")
    return value


def parse_header(text: str) -> Header:
    """Prototypes of the pit_* entries, struct layouts and object-like integer PIT_* #defines of a C header's text.  Anything
    else in it (beside comments, other preprocessor lines, forward declarations and the extern "C" braces) raises."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text.replace("\\\n", " "), flags=re.S)
    defines = {}
    for name, paren, body in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PIT_\w+)(\(?)([^\n]*)$", text, flags=re.M):
        if not paren and body.strip():        # (function-like macros and the empty include guard are not values)
            defines[name] = _evaluate(body, defines, name)
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)
    structs = {}

    def struct(m) -> str:
        where = f"struct {m.group(1)}"
        structs[m.group(1)] = [f for decl in m.group(2).split(";") if decl.strip() for f in _declarators(decl, where)]
        return " "
    text = re.sub(r"(?:typedef\s+)?struct\s+(\w+)\s*\{(.*?)\}\s*\w*\s*;", struct, text, flags=re.S)
    prototypes = {}
    for stmt in text.split(";"):
        stmt = stmt.strip().lstrip("}").strip()               # (the extern "C" block's closing brace)
        if not stmt or re.fullmatch(r"struct\s+\w+", stmt):
            continue
        m = re.fullmatch(r"([\w\s*]+?)\s*\b(pit_\w+)\s*\(([^()]*)\)", stmt, flags=re.S)
        if not m:
            raise ValueError(f"cannot parse the declaration {' '.join(stmt.split())[:80]!r}")
        ret, name, params = m.groups()
        ret = re.sub(r"\s*\*", "*", " ".join(ret.split()))
        if ret not in _RETURNS:
            raise ValueError(f"{name}: no ctypes type for the return type {ret!r}")
        args = [] if params.strip() == "void" else [a for p in params.split(",") for a in _declarators(p, name)]
        prototypes[name] = Prototype(_RETURNS[ret], [t for _, t in args], [n for n, _ in args])
    return Header(prototypes, structs, defines)


try:
    with open(HEADER_PATH) as _f:
        _HEADER = parse_header(_f.read())
except OSError as _e:
    raise RuntimeError(f"{HEADER_PATH} not found: the binding is derived from it ({_e})") from None

PROTOTYPES = _HEADER.prototypes                                           # name -> (restype, argtypes, argnames)
SIGNATURES = {name: p.argtypes for name, p in PROTOTYPES.items()}         # name -> argtypes
LONG_RETURN = {name for name, p in PROTOTYPES.items() if p.restype is ctypes.c_long}
DEFINES = types.MappingProxyType(_HEADER.defines)                         # the header's own names -> values, read-only


class MlpParamsJob(ctypes.Structure):
    """pit_mlp_params_job of include/pit_hip.h (the argument list of pit_mlp_bwd_params)."""
    _fields_ = _HEADER.structs["pit_mlp_params_job"]


class BlockWeightsJob(ctypes.Structure):
    """pit_block_weights_job of include/pit_hip.h (the argument list of pit_block_weights)."""
    _fields_ = _HEADER.structs["pit_block_weights_job"]


class SlabPlan(ctypes.Structure):
    """pit_slab_plan of include/pit_hip.h (the static per-slab plan of a masked cross-attention layer on a fixed mesh pair)."""
    _fields_ = _HEADER.structs["pit_slab_plan"]


class DecoderWeightsJob(ctypes.Structure):
    """pit_decoder_weights_job of include/pit_hip.h (the argument list of pit_decoder_weights)."""
    _fields_ = _HEADER.structs["pit_decoder_weights_job"]


# entries added to an ABI version after its first release (PIT_HAS_* in the header): a library of the same version built before
# them lacks the symbols
ADDED_LATER = {"pit_distlist_select_fwd", "pit_distlist_fwd", "pit_distlist_bwd_workspace", "pit_distlist_bwd",
               "pit_rel_lp_loss_ragged_fwd_grad", "pit_rel_max_norm_ragged",       # PIT_HAS_DISTLIST, PIT_HAS_RAGGED_STEP
               "pit_block_fwd_set_form", "pit_block_fwd_last_rows",                # PIT_HAS_BLOCK_ROWS8
               "pit_block_bwd_last_riders",                                        # PIT_HAS_RIDER_TAIL
               "pit_posatt_dhead_finish_stage", "pit_finish_last_tail",            # PIT_HAS_FINISH_TAIL
               "pit_debug_att_counts",                                             # PIT_HAS_ATT_COUNTS
               "pit_debug_dense_counts",                                           # PIT_HAS_DENSE_COUNTS
               "pit_eval_metrics_workspace", "pit_eval_metrics",                   # PIT_HAS_EVAL_METRICS
               "pit_batch_feed",                                                   # PIT_HAS_BATCH_FEED
               "pit_adam_guard_parts", "pit_adam_step_guarded",                    # PIT_HAS_GUARDED_ADAM
               "pit_adam_step_averaged", "pit_exchange_words",                     # PIT_HAS_AVERAGED_ADAM
               "pit_fps",                                                          # PIT_HAS_FPS
               "pit_batch_feed_points",                                            # PIT_HAS_FEED_POINTS
               "pit_fps_large_workspace", "pit_fps_large",                         # PIT_HAS_FPS_LARGE
               "pit_knn_box", "pit_knn_rows", "pit_knn_last_form",                 # PIT_HAS_KNN
               "pit_distlist_select_ragged_fwd", "pit_distlist_ragged_fwd", "pit_distlist_ragged_bwd",      # PIT_HAS_DISTLIST_RAGGED
               "pit_knn_box_ragged",                                               # PIT_HAS_KNN_RAGGED
               "pit_geo_knn"}                                                      # PIT_HAS_GEO
ABI_VERSION = DEFINES["PIT_ABI_VERSION"]      # of the header this checkout carries; lib() holds the loaded library to it
FPS_MAX_POINTS = DEFINES["PIT_FPS_MAX_POINTS"]
FPS_MAX_POINTS_WIDE = DEFINES["PIT_FPS_MAX_POINTS_WIDE"]          # (space_dim 4..8)
FPS_LARGE_MAX_POINTS = DEFINES["PIT_FPS_LARGE_MAX_POINTS"]        # (every space_dim)
FPS_LARGE_MAX_SAMPLES = DEFINES["PIT_FPS_LARGE_MAX_SAMPLES"]
KNN_MAX_K = DEFINES["PIT_KNN_MAX_K"]
KNN_REG_MAX_KEYS = DEFINES["PIT_KNN_REG_MAX_KEYS"]
GEO_MAX_K = DEFINES["PIT_GEO_MAX_K"]
GEO_MAX_REACH = DEFINES["PIT_GEO_MAX_REACH"]
GUARD_MAX_PARTS = DEFINES["PIT_GUARD_MAX_PARTS"]
GUARD_STATE_DOUBLES = DEFINES["PIT_GUARD_STATE_DOUBLES"]
FEED_MAX_FIELDS = DEFINES["PIT_FEED_MAX_FIELDS"]
FEED_MAX_ROW_BYTES = DEFINES["PIT_FEED_MAX_ROW_BYTES"]
FEED_WHOLE_ROW = DEFINES["PIT_FEED_WHOLE_ROW"]
FEED_POINTS_G0 = DEFINES["PIT_FEED_POINTS_G0"]
FEED_POINTS_G1 = DEFINES["PIT_FEED_POINTS_G1"]
EVAL_STATE_DOUBLES = DEFINES["PIT_EVAL_STATE_DOUBLES"]
EVAL_MAX_PARTS = DEFINES["PIT_EVAL_MAX_PARTS"]
DISTLIST_CHUNK = DEFINES["PIT_DISTLIST_CHUNK"]


def distlist_chunk_slots(n_out: int, cap: int) -> int:
    """PIT_DISTLIST_CHUNK_SLOTS of include/pit_hip.h (a function-like macro: written out here, checked against a compiler by the
    tests)."""
    return int(n_out) * int(cap) // (DISTLIST_CHUNK // 2) + 1


_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -m position_induced_transformer_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback for the PiT hot path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, proto in PROTOTYPES.items():
            try:
                fn = getattr(handle, name)   # AttributeError if the ABI lost a symbol
            except AttributeError:
                if name not in ADDED_LATER:
                    raise
                raise RuntimeError(f"{LIB_PATH} was built before {name} joined PIT_ABI_VERSION {ABI_VERSION}: "
                                   "rebuild it (python -m position_induced_transformer_amd.build)") from None
            fn.argtypes = proto.argtypes
            fn.restype = proto.restype
        got = handle.pit_version()           # the default library and a PIT_LIB_PATH override alike
        if got != ABI_VERSION:
            raise RuntimeError(f"{LIB_PATH} implements PIT_ABI_VERSION {got}, this package binds version {ABI_VERSION}: "
                               "rebuild it (python -m position_induced_transformer_amd.build)")
        _lib = handle
    return _lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = lib().pit_error_string(code)
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else '?'}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


# ---- argument groups that recur in the layer entries beside the main mesh path (ragged, distance matrix, candidate lists), in the
# header's parameter order (t: a (batch, points, channels) tensor whose rows are contiguous) ---------------------------------------
def values_args(t, with_batch: bool) -> tuple:
    """values, [batch,] dim, ld_values, values_bstride"""
    b, _, d = t.shape
    return (t.data_ptr(),) + ((b, d) if with_batch else (d,)) + (t.stride(1), t.stride(0))


def head_args(head, n_head: int, is_scale: bool, *scale) -> tuple:
    """head, n_head, head_is_scale; with the forward's scale_out as ``scale``: ..., scale"""
    return (head.data_ptr(), n_head, 1 if is_scale else 0) + tuple(c.data_ptr() for c in scale)


def out_args(out, d: int, concat: bool, rowstat, scale_out) -> tuple:
    """out, ld_out, out_bstride, out_col0, copy_inputs, rowstat, scale_out"""
    return (out.data_ptr(), out.stride(1), out.stride(0), d if concat else 0, 1 if concat else 0, rowstat.data_ptr(), scale_out.data_ptr())


def dout_args(d_out, d: int, concat: bool) -> tuple:
    """d_out, ld_dout, dout_bstride, out_col0"""
    return (d_out.data_ptr(), d_out.stride(1), d_out.stride(0), d if concat else 0)


def dvalues_args(d_values, j: int, d: int, concat: bool) -> tuple:
    """d_values, ld_dvalues, dvalues_bstride, add_residual"""
    return (ptr(d_values), d, j * d, 1 if concat else 0)


def dhead_args(d_head, workspace) -> tuple:
    """d_head, accumulate_head, workspace"""
    return (ptr(d_head), 0, ptr(workspace))


def saved_out_args(out) -> tuple:
    """out, ld_out, out_bstride (the forward's result, read by d(m) / d(sqd))"""
    return (None, 0, 0) if out is None else (out.data_ptr(), out.stride(1), out.stride(0))
