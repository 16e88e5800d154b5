"""The C-ABI of the motion clip without a GPU: include/trex_motion.h is reached through include/trex_batch.h and stands alone, both
as C; the library exports what it declares; and the ctypes signature table of trex_gym.motion_capi agrees with the header - the
number of parameters, and a pointer for a pointer, the scalar of the same width for a scalar (the check
tests/test_reward_capi_host.py makes for trex_reward.h)."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
NAMES = ["trex_batch_set_motion", "trex_batch_motion_info", "trex_batch_motion_sample", "trex_batch_set_motion_reward",
         "trex_batch_compose_motion_reward", "trex_batch_motion_reset"]


def declarations():
    """[(name, return type, [parameter, ...])] of every trex_* function trex_motion.h declares, as normalised C text"""
    text = open(os.path.join(INCLUDE, "trex_motion.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[^\n]*", " ", text, flags=re.M)
    out = []
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(trex_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        out.append((name, " ".join(ret.split()), [" ".join(p.split()) for p in params.split(",")]))
    return out


def test_header_declares_the_six_calls_and_the_library_exports_them():
    from trex_gym import _capi, motion_capi, reward_capi
    assert [d[0] for d in declarations()] == NAMES == motion_capi.MOTION_SYMBOLS
    assert not set(NAMES) & (set(_capi.SYMBOLS) | set(reward_capi.REWARD_SYMBOLS))
    for name in NAMES:
        assert hasattr(_capi.lib, name), name
    assert '#include "trex_motion.h"' in open(os.path.join(INCLUDE, "trex_batch.h")).read()


def test_signature_table_matches_the_header():
    from trex_gym import _capi, motion_capi
    scalars = {"int": (C.c_int, C.c_int32), "int32_t": (C.c_int, C.c_int32), "uint32_t": (C.c_uint32,), "float": (C.c_float,),
               "double": (C.c_double,)}
    is_pointer = lambda t: t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))
    wrong = []
    for name, ret, params in declarations():
        restype, argtypes = motion_capi._MOTION_API[name]
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
    assert C.sizeof(motion_capi.TrexMotionTerm) == 20                 # int32, uint32, 3 floats


def test_either_header_alone_declares_both_as_c(tmp_path):
    for first in ("trex_motion.h", "trex_batch.h"):
        src = tmp_path / ("use_%s.c" % first[:-2])
        src.write_text('#include "%s"\n'
                       "int use(TrexBatch *b, float *rows, const double *f, const TrexMotionTerm *t) {\n"
                       "  return trex_batch_set_motion(b, f, 0, 2, 0.5, 0, -1) + trex_batch_set_motion_reward(b, t, TREX_MOT_KINDS, 1.0f) +\n"
                       "         trex_batch_compose_motion_reward(b, rows, 77, 0, 0) + trex_batch_motion_reset(b, 0, 0, rows, 77, 0) +\n"
                       "         trex_batch_motion_sample(b, 0, rows, 0, 0, 0) + trex_batch_motion_info(b, 0, 0, 0, 0) +\n"
                       "         trex_batch_num_envs(b) + trex_batch_reward_terms(b);\n}\n" % first)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])
