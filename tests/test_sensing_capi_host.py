"""The C-ABI of the sensor model without a GPU: include/trex_sensing.h is reached through include/trex_batch.h and stands alone,
both as C; the library exports what it declares; and the ctypes signature table of trex_gym.sensing_capi agrees with the header -
the number of parameters, and a pointer for a pointer, the scalar of the same width for a scalar (the check
tests/test_motion_capi_host.py makes for trex_motion.h)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
NAMES = ["trex_batch_set_sensing", "trex_batch_apply_sensing", "trex_batch_sensing_reset", "trex_batch_set_action_delay",
         "trex_batch_delay_actions", "trex_batch_sensing_info"]


def declarations():
    """[(name, return type, [parameter, ...])] of every trex_* function trex_sensing.h declares, as normalised C text"""
    text = open(os.path.join(INCLUDE, "trex_sensing.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(trex_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        out.append((name, " ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")]))
    return out


def test_header_declares_the_six_calls_and_the_library_exports_them():
    from trex_gym import _capi, motion_capi, reward_capi, sensing_capi
    assert [d[0] for d in declarations()] == NAMES == sensing_capi.SENSING_SYMBOLS
    assert not set(NAMES) & (set(_capi.SYMBOLS) | set(reward_capi.REWARD_SYMBOLS) | set(motion_capi.MOTION_SYMBOLS))
    for name in NAMES:
        assert hasattr(_capi.lib, name), name
    text = open(os.path.join(INCLUDE, "trex_batch.h")).read()
    assert text.index('#include "trex_motion.h"') < text.index('#include "trex_sensing.h"') < text.index("#endif /* TREX_BATCH_H */")


def test_signature_table_matches_the_header():
    from trex_gym import _capi, sensing_capi
    scalars = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "uint32_t": (C.c_uint32,), "uint64_t": (C.c_uint64,),
               "float": (C.c_float,), "double": (C.c_double,)}
    is_pointer = lambda t: t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))
    wrong = []
    for name, ret, params in declarations():
        restype, argtypes = sensing_capi._SENSING_API[name]
        fn = getattr(_capi.lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
        if ret != "int" or restype is not C.c_int:
            wrong.append("%s: returns `%s`, restype %s" % (name, ret, restype))
        if len(params) != len(argtypes):
            wrong.append("%s: %d parameters declared, %d argtypes" % (name, len(params), len(argtypes)))
            continue
        for k, (p, a) in enumerate(zip(params, argtypes)):
            if "*" in p:
                ok = is_pointer(a)
            else:
                words = [w for w in p.split() if w != "const"]
                ok = len(words) == 2 and a in scalars[words[0]]
            if not ok:
                wrong.append("%s: parameter %d `%s` is bound as %s" % (name, k, p, a))
    assert not wrong, "\n".join(wrong)
    assert C.sizeof(sensing_capi.TrexSenseGroup) == 32                 # 3 int32, 3 floats, 2 int32


def test_struct_and_constants_match_the_header():
    from trex_gym import sensing_capi
    text = open(os.path.join(INCLUDE, "trex_sensing.h")).read()
    body = re.sub(r"/\*.*?\*/", " ", re.search(r"typedef struct TrexSenseGroup \{(.*?)\} TrexSenseGroup;", text, re.S).group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        fields += [(w, words[0]) for w in words[1:]]
    ctype = {"int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for n, t in fields] == list(sensing_capi.TrexSenseGroup._fields_)
    define = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))
    assert (define("TREX_SENSE_GAUSSIAN"), define("TREX_SENSE_UNIFORM")) == (sensing_capi.GAUSSIAN, sensing_capi.UNIFORM)
    assert (define("TREX_SENSE_MAXDELAY"), define("TREX_SENSE_MAXGROUPS")) == (sensing_capi.MAX_DELAY, sensing_capi.MAX_GROUPS)
    limits = open(os.path.join(ROOT, "trex-gym_amd", "csrc", "sensing_limits.h")).read()
    assert int(re.search(r"#define TREX_SENSE_SLOTS (\d+)", limits).group(1)) == sensing_capi.MAX_DELAY + 1


def test_either_header_alone_declares_both_as_c(tmp_path):
    for first in ("trex_sensing.h", "trex_batch.h"):
        src = tmp_path / ("use_%s.c" % first[:-2])
        src.write_text('#include "%s"\n'
                       "int use(TrexBatch *b, float *rows, const TrexSenseGroup *g, int32_t *d) {\n"
                       "  return trex_batch_set_sensing(b, g, TREX_SENSE_MAXGROUPS, 1u, 0u) + trex_batch_apply_sensing(b, rows, 77, rows, 77, 0) +\n"
                       "         trex_batch_sensing_reset(b, 0, 0) + trex_batch_set_action_delay(b, 0, TREX_SENSE_MAXDELAY) +\n"
                       "         trex_batch_delay_actions(b, rows, 0, rows, 0) + trex_batch_sensing_info(b, 0, 0, 0, 0, d, d, 0) +\n"
                       "         trex_batch_num_envs(b) + trex_batch_motion_info(b, 0, 0, 0, 0) + TREX_SENSE_UNIFORM;\n}\n" % first)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])
