"""No GPU: the ctypes binding that _lib derives from include/pit_hip.h.  A host C++ compiler states what the header means (every
entry's parameter and return types, struct sizes and field offsets, the value of every integer #define, PIT_DISTLIST_CHUNK_SLOTS)
and the derived binding must say the same; the parser on hostile header text; the argument-group builders against the header's
parameter names; the built library exports no pit_* symbol the header does not declare."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "pit_hip.h")

# the probe's codes -> ctypes (where long and long long have one size ctypes makes them one type, as the ABI does)
CODES = {"P": ctypes.c_void_p, "I": ctypes.c_int, "L": ctypes.c_long, "LL": ctypes.c_longlong, "F": ctypes.c_float,
         "D": ctypes.c_double, "S": ctypes.c_char_p}
STRUCTS = {"pit_mlp_params_job": "MlpParamsJob", "pit_block_weights_job": "BlockWeightsJob", "pit_slab_plan": "SlabPlan",
           "pit_decoder_weights_job": "DecoderWeightsJob"}
# (n_out, cap) of PIT_DISTLIST_CHUNK_SLOTS: the smallest, either side of the first step (CHUNK / 2 = 256 slots), an odd pair, and
# the largest the list layers accept (cap <= PIT_DISTLIST_MAX_CAP = 2048, n_out * cap < 2^31)
CHUNK_PAIRS = [(1, 1), (255, 1), (256, 1), (257, 3), (4097, 64), ((2 ** 31 - 1) // 2048, 2048), (2 ** 31 - 1, 1)]

PROBE_HEAD = r"""
#include <cstddef>
#include <cstdio>
#include "pit_hip.h"
template <class T> struct arg;                       /* a type outside the binding's map does not compile */
template <class T> struct arg<T*> { static const char* s() { return "P"; } };
template <> struct arg<int> { static const char* s() { return "I"; } };
template <> struct arg<long> { static const char* s() { return "L"; } };
template <> struct arg<long long> { static const char* s() { return "LL"; } };
template <> struct arg<float> { static const char* s() { return "F"; } };
template <> struct arg<double> { static const char* s() { return "D"; } };
template <class T> struct ret;
template <> struct ret<int> { static const char* s() { return "I"; } };
template <> struct ret<long> { static const char* s() { return "L"; } };
template <> struct ret<const char*> { static const char* s() { return "S"; } };
template <class F> struct sig;
template <class R, class... A> struct sig<R(A...)> {
    static void print(const char* name) {
        const char* a[] = {arg<A>::s()..., 0};
        std::printf("sig %s %s", name, ret<R>::s());
        for (int i = 0; a[i]; ++i) std::printf(" %s", a[i]);
        std::printf("\n");
    }
};
int main() {
"""


def host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx.split()[0]):
            return cxx.split()
    return None


def header_code() -> str:
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """What a host C++ compiler makes of the header, as {first two words of a line: the rest of its words}.  The names of
    entries and #defines come from plain regular expressions on the header here, not from _lib's parser."""
    from position_induced_transformer_amd import _lib
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (CXX, c++, g++, clang++)")
    code = header_code()
    entries = sorted(set(re.findall(r"\b(pit_[a-z0-9_]+)\s*\(", code)))
    defines = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(PIT_\w+)[ \t]+\S", code, flags=re.M)
    lines = [PROBE_HEAD]
    lines += [f'    sig<decltype({e})>::print("{e}");' for e in entries]
    for c_name, cls in STRUCTS.items():
        fields = [n for n, _ in getattr(_lib, cls)._fields_]
        lines.append(f'    std::printf("struct {c_name} %zu\\n", sizeof({c_name}));')
        lines += [f'    std::printf("field {c_name}.{f} %zu %zu\\n", offsetof({c_name}, {f}), sizeof((({c_name}*)0)->{f}));' for f in fields]
    lines += [f'    std::printf("define {d} %lld\\n", (long long)({d}));' for d in defines]
    lines += [f'    std::printf("chunk_slots {n},{c} %lld\\n", (long long)PIT_DISTLIST_CHUNK_SLOTS({n}, {c}));' for n, c in CHUNK_PAIRS]
    lines.append("    return 0;\n}\n")
    tmp = tmp_path_factory.mktemp("abi_probe")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text("\n".join(lines))
    subprocess.run(cxx + ["-std=c++14", "-I", INCLUDE, str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    table = {}
    for line in out.splitlines():
        kind, key, *rest = line.split()
        table.setdefault(kind, {})[key] = rest
    table["entries"], table["define_names"] = entries, defines
    return table


def test_compiler_probe_agrees_on_every_entry(probe):
    from position_induced_transformer_amd import _lib
    assert sorted(_lib.SIGNATURES) == probe["entries"] == sorted(probe["sig"]) and len(probe["entries"]) >= 109
    for name in probe["entries"]:
        proto = _lib.PROTOTYPES[name]
        assert [proto.restype] + proto.argtypes == [CODES[c] for c in probe["sig"][name]], name
        assert _lib.SIGNATURES[name] == proto.argtypes and len(proto.argnames) == len(proto.argtypes), name
        assert (name in _lib.LONG_RETURN) == (probe["sig"][name][0] == "L"), name
    assert _lib.PROTOTYPES["pit_error_string"].restype is ctypes.c_char_p


def test_compiler_probe_agrees_on_every_struct(probe):
    from position_induced_transformer_amd import _lib
    for c_name, cls_name in STRUCTS.items():
        cls = getattr(_lib, cls_name)
        assert ctypes.sizeof(cls) == int(probe["struct"][c_name][0]), c_name
        for field, ctype in cls._fields_:
            offset, size = (int(v) for v in probe["field"][f"{c_name}.{field}"])
            assert (getattr(cls, field).offset, ctypes.sizeof(ctype)) == (offset, size), (c_name, field)
        # the fields tile the struct up to alignment padding: none was missed in between or at the end
        end = max(getattr(cls, f).offset + ctypes.sizeof(t) for f, t in cls._fields_)
        assert ctypes.sizeof(cls) - end < ctypes.alignment(cls), c_name


def test_compiler_probe_agrees_on_every_define(probe):
    from position_induced_transformer_amd import _lib, ops
    assert sorted(_lib.DEFINES) == sorted(probe["define_names"]) and len(probe["define_names"]) >= 140
    for name in probe["define_names"]:
        assert _lib.DEFINES[name] == int(probe["define"][name][0]), name
    with pytest.raises(TypeError):
        _lib.DEFINES["PIT_ABI_VERSION"] = 0                     # read-only
    for attr in ("ABI_VERSION", "FPS_MAX_POINTS", "FPS_MAX_POINTS_WIDE", "FPS_LARGE_MAX_POINTS", "FPS_LARGE_MAX_SAMPLES", "KNN_MAX_K",
                 "KNN_REG_MAX_KEYS", "GUARD_MAX_PARTS", "GUARD_STATE_DOUBLES", "FEED_MAX_FIELDS", "FEED_MAX_ROW_BYTES", "FEED_WHOLE_ROW",
                 "FEED_POINTS_G0", "FEED_POINTS_G1", "EVAL_STATE_DOUBLES", "EVAL_MAX_PARTS", "DISTLIST_CHUNK"):
        assert getattr(_lib, attr) == int(probe["define"]["PIT_" + attr][0]), attr
    value = lambda name: int(probe["define"][name][0])   # noqa: E731
    assert ops.METRIC_ID == {"euclid": value("PIT_METRIC_EUCLID"), "periodic1d": value("PIT_METRIC_PERIODIC1D"),
                             "periodic2d": value("PIT_METRIC_PERIODIC2D")}
    assert ops.MATH_MODES == {"fp32": value("PIT_MATH_FP32"), "bf16": value("PIT_MATH_BF16")}
    for attr, name in (("MAX_SPACE_DIM", "PIT_MAX_SPACE_DIM"), ("IO_X_BF16", "PIT_IO_X_BF16"), ("IO_SAVE_BF16", "PIT_IO_SAVE_BF16"),
                       ("IO_DX_BF16", "PIT_IO_DX_BF16"), ("IO_OUT_BF16", "PIT_IO_OUT_BF16"), ("IO_DOUT_BF16", "PIT_IO_DOUT_BF16"),
                       ("ATT_UNION", "PIT_ATT_UNION"), ("SLAB_UNION_MAX", "PIT_SLAB_UNION_MAX"), ("LIST_MAX_CAP", "PIT_DISTLIST_MAX_CAP"),
                       ("KNN_MAX_K", "PIT_KNN_MAX_K"), ("KNN_REG_MAX_KEYS", "PIT_KNN_REG_MAX_KEYS")):
        assert getattr(ops, attr) == value(name), attr


def test_compiler_probe_agrees_on_distlist_chunk_slots(probe):
    from position_induced_transformer_amd import _lib
    for n_out, cap in CHUNK_PAIRS:
        assert _lib.distlist_chunk_slots(n_out, cap) == int(probe["chunk_slots"][f"{n_out},{cap}"][0]), (n_out, cap)
    assert _lib.distlist_chunk_slots(255, 1) == 1 and _lib.distlist_chunk_slots(256, 1) == 2


# ----------------------------------------------------------------------------- the parser on hostile text
HOSTILE = """
/* pit_commented(a, b);  and
#define PIT_COMMENTED 3
*/
#define PIT_GUARD_H
#define PIT_A 0x10          /* pit_also_commented(int a); */
#define PIT_B (PIT_A << 2 | 1)
#define PIT_C (1L << 30)
#define PIT_D -2
#define PIT_E 3U * (PIT_A - 1) + 2 & 0xff
#define PIT_FN(a, b) ((a) * PIT_A + (b))
// #define PIT_LINE_COMMENTED 5
struct pit_job;
typedef struct pit_plan { int n, m, cap; const float* stats; float w; } pit_plan;
struct pit_job {
    const pit_plan* plan; const float* const* heads; int a, b;
    float *e, *q; double d; long long count; long ld;
};
int pit_spread(const float* x,
               long ld_x /* a comment
               that runs on */, double* const* parts,
               long long n,
               const struct pit_job* job);
long pit_bytes(void);
const char* pit_text(int code);
"""


def test_parser_on_hostile_text():
    from position_induced_transformer_amd import _lib
    P, I, L, LL, F, D = (ctypes.c_void_p, ctypes.c_int, ctypes.c_long, ctypes.c_longlong, ctypes.c_float, ctypes.c_double)
    h = _lib.parse_header(HOSTILE)
    assert h.defines == {"PIT_A": 16, "PIT_B": 65, "PIT_C": 1 << 30, "PIT_D": -2, "PIT_E": (3 * 15 + 2) & 0xff}
    assert sorted(h.prototypes) == ["pit_bytes", "pit_spread", "pit_text"]
    assert h.prototypes["pit_spread"] == (I, [P, L, P, LL, P], ["x", "ld_x", "parts", "n", "job"])
    assert h.prototypes["pit_bytes"] == (L, [], [])
    assert h.prototypes["pit_text"] == (ctypes.c_char_p, [I], ["code"])
    assert h.structs == {"pit_plan": [("n", I), ("m", I), ("cap", I), ("stats", P), ("w", F)],
                         "pit_job": [("plan", P), ("heads", P), ("a", I), ("b", I), ("e", P), ("q", P), ("d", D), ("count", LL),
                                     ("ld", L)]}


@pytest.mark.parametrize("text,names", [
    ("int pit_x(const float* a, short n);", ("pit_x", "short")),                    # an unknown scalar: never defaulted
    ("int pit_x(unsigned n);", ("pit_x", "unsigned")),
    ("int pit_x();", ("pit_x",)),                                                   # C's unspecified parameters: (void) is the empty list
    ("int pit_x(int);", ("pit_x",)),                                                # no parameter name: no type is left
    ("float pit_x(int n);", ("pit_x", "float")),                                    # a return type outside int / long / const char*
    ("void pit_x(int n);", ("pit_x", "void")),
    ("struct pit_s { int a; short b; };", ("pit_s", "short")),
    ("int pit_x(int (*callback)(int));", ("pit_x",)),
    ("int pit_x(int n) { return n; }", ("pit_x",)),                                 # not a declaration
    ("#define PIT_Y sizeof(int)", ("PIT_Y",)),                                      # a call
    ("#define PIT_Y 3 / 2", ("PIT_Y",)),                                            # an operator outside the list
    ("#define PIT_Y 1.5", ("PIT_Y",)),
    ("#define PIT_Y (PIT_LATER + 1)\n#define PIT_LATER 2", ("PIT_Y", "PIT_LATER")),  # only EARLIER names are known
    ("#define PIT_Y (1 << 2", ("PIT_Y",)),
    ("#define PIT_Y 1 +", ("PIT_Y",)),
    ("#define PIT_Y OTHER_NAME", ("PIT_Y",)),
])
def test_parser_raises_and_names_what_it_cannot_read(text, names):
    from position_induced_transformer_amd import _lib
    with pytest.raises(ValueError) as err:
        _lib.parse_header(text)
    for name in names:
        assert name in str(err.value), (name, str(err.value))


def test_header_is_found_beside_the_package_and_parsed_at_import_only(monkeypatch):
    from position_induced_transformer_amd import _lib, build
    assert os.path.samefile(_lib.HEADER_PATH, HEADER)
    assert _lib.ABI_VERSION == _lib.DEFINES["PIT_ABI_VERSION"]
    build.build()                                                  # no-op when up to date
    monkeypatch.setattr(_lib, "parse_header", lambda text: pytest.fail("lib() parsed the header again"))
    monkeypatch.setattr(_lib, "_lib", None)                        # a first lib() call: loads and binds from what import derived
    assert _lib.lib().pit_version() == _lib.ABI_VERSION
    assert _lib.lib().pit_posatt_fwd.argtypes == _lib.SIGNATURES["pit_posatt_fwd"]
    assert _lib.lib().pit_satt_tiles_elems.restype is ctypes.c_long and _lib.lib().pit_error_string.restype is ctypes.c_char_p


# ----------------------------------------------------------------------------- the builders against the header's names
RAGGED = ["pit_posatt_ragged_", "pit_posatt_ragged_strided_"]
SUPPLIED = ["pit_distmat_", "pit_distlist_"]
FWD = [e + "fwd" for e in RAGGED + SUPPLIED]
BWD = [e + "bwd" for e in RAGGED + SUPPLIED]
BUILDER_RUNS = [       # builder, the parameter names it produces in order, the entries whose call in ops.py spreads it
    ("values_args", ["values", "dim", "ld_values", "values_bstride"], [e + d for e in RAGGED for d in ("fwd", "bwd")]),
    ("values_args", ["values", "batch", "dim", "ld_values", "values_bstride"], [e + d for e in SUPPLIED for d in ("fwd", "bwd")]),
    ("head_args", ["head", "n_head", "head_is_scale"], FWD),
    ("head_args", ["head", "n_head", "head_is_scale", "scale"], BWD),
    ("out_args", ["out", "ld_out", "out_bstride", "out_col0", "copy_inputs", "rowstat", "scale_out"], FWD),
    ("dout_args", ["d_out", "ld_dout", "dout_bstride", "out_col0"], BWD),
    ("dvalues_args", ["d_values", "ld_dvalues", "dvalues_bstride", "add_residual"], BWD),
    ("dhead_args", ["d_head", "accumulate_head", "workspace"], BWD),
    ("saved_out_args", ["out", "ld_out", "out_bstride"], ["pit_distmat_bwd", "pit_distlist_bwd"]),
]


class FakeTensor:
    """Enough of a (batch, points, channels) tensor for the builders: distinct values for pointer, sizes and strides."""
    shape = (5, 7, 3)

    def __init__(self, address):
        self.address = address

    def data_ptr(self):
        return self.address

    def stride(self, axis):
        return (21, 3, 1)[axis]


@pytest.mark.parametrize("builder,run,entries", BUILDER_RUNS, ids=[f"{b}-{len(r)}" for b, r, _ in BUILDER_RUNS])
def test_builders_follow_the_headers_parameter_names(builder, run, entries):
    from position_induced_transformer_amd import _lib
    for entry in entries:
        names = _lib.PROTOTYPES[entry].argnames
        starts = [i for i in range(len(names) - len(run) + 1) if names[i:i + len(run)] == run]
        assert len(starts) == 1, (entry, run, names)               # contiguous, and in one place only
        # the run's types are what the builder's values must convert to: pointers then sizes / strides
        types = _lib.SIGNATURES[entry][starts[0]:starts[0] + len(run)]
        assert types[0] is ctypes.c_void_p, (entry, run)
    t = FakeTensor(1000)
    made = {"values_args": lambda: _lib.values_args(t, "batch" in run),
            "head_args": lambda: _lib.head_args(t, 2, True, *([FakeTensor(2000)] if "scale" in run else [])),
            "out_args": lambda: _lib.out_args(t, 3, True, FakeTensor(3000), FakeTensor(4000)),
            "dout_args": lambda: _lib.dout_args(t, 3, True),
            "dvalues_args": lambda: _lib.dvalues_args(t, 7, 3, True),
            "dhead_args": lambda: _lib.dhead_args(t, FakeTensor(5000)),
            "saved_out_args": lambda: _lib.saved_out_args(t)}[builder]()
    want = {"values": 1000, "batch": 5, "dim": 3, "ld_values": 3, "values_bstride": 21, "head": 1000, "n_head": 2, "head_is_scale": 1,
            "scale": 2000, "out": 1000, "ld_out": 3, "out_bstride": 21, "out_col0": 3, "copy_inputs": 1, "rowstat": 3000,
            "scale_out": 4000, "d_out": 1000, "ld_dout": 3, "dout_bstride": 21, "d_values": 1000, "ld_dvalues": 3,
            "dvalues_bstride": 21, "add_residual": 1, "d_head": 1000, "accumulate_head": 0, "workspace": 5000}
    assert list(made) == [want[name] for name in run], (builder, run)


# ----------------------------------------------------------------------------- the library exports nothing undeclared
def test_library_exports_no_undeclared_pit_symbol():
    from position_induced_transformer_amd import _lib, build
    build.build()                                                  # no-op when up to date
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin")
    if nm is None:
        pytest.skip("neither nm nor llvm-nm on this machine")
    out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("pit_")}
    assert exported, "nm listed no pit_* export"
    assert exported - set(_lib.SIGNATURES) == set(), "exported but not declared in pit_hip.h"
    assert set(_lib.SIGNATURES) - exported == set()
