"""The public Python surface of the episode monitor, recorded like the one tests/test_randomize_surface.py keeps for the episode
randomisation: every public name of trex_gym.monitor and trex_gym.monitor_capi with its signature, the public methods of
BatchMonitor, the summary's field indices, and the attributes a TrexVecEnv with a monitor attached carries on the instance - against
tests/golden/monitor_surface.json. Host-only: nothing is constructed.

A pull request that moves this surface rewrites the record in the same commit:  python tests/test_monitor_surface.py"""
import inspect
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor_surface.json")
ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def _describe(value):
    if inspect.isclass(value):
        return "class"
    if callable(value):
        return str(inspect.signature(value))
    return "attribute: " + type(value).__name__


def _members(cls):
    out = {}
    for a in sorted(dir(cls)):
        if not a.startswith("_"):
            v = inspect.getattr_static(cls, a)
            out[a] = "property" if isinstance(v, property) else _describe(getattr(cls, a))
    return out


def surface():
    from trex_gym import monitor, monitor_capi, vec_env
    out = {}
    for mod in (monitor, monitor_capi):
        own = {a: v for a, v in vars(mod).items() if not a.startswith("_") and not inspect.ismodule(v)
               and getattr(v, "__module__", mod.__name__) == mod.__name__}
        out[mod.__name__] = {a: _describe(v) for a, v in sorted(own.items())}
    out["trex_gym.monitor_capi.BatchMonitor"] = _members(monitor_capi.BatchMonitor)
    out["trex_gym.monitor_capi.MONITOR_SYMBOLS"] = list(monitor_capi.MONITOR_SYMBOLS)
    out["trex_gym.monitor_capi summary fields"] = {k: getattr(monitor_capi, k) for k in (
        "N", "RET_MEAN", "RET_MIN", "RET_MAX", "LEN_MEAN", "LEN_MIN", "LEN_MAX", "WIN_REASON", "TOTAL", "BY_REASON", "T", "SUMMARY")}
    out["trex_gym.monitor_capi info buffers"] = [list(f) for f in monitor_capi.RING_FIELDS + monitor_capi.ENV_FIELDS]
    out["trex_gym.monitor_capi.REASON_NAMES"] = list(monitor_capi.REASON_NAMES)
    # what the env carries for the monitor (instance attributes do not show in dir(class))
    src = inspect.getsource(vec_env.TrexVecEnv.__init__) + inspect.getsource(vec_env.TrexVecEnv._set_monitor)
    out["trex_gym.vec_env.TrexVecEnv instance"] = sorted(a for a in set(re.findall(r"self\.([a-z]\w*)\b(?=[^=\n]*=[^=])", src))
                                                        if a.startswith("monitor"))
    out["trex_gym.vec_env.TrexVecEnv._set_monitor"] = str(inspect.signature(vec_env.TrexVecEnv._set_monitor))
    return out


def test_monitor_surface_is_the_recorded_one():
    want, got = json.load(open(GOLDEN)), surface()
    diff = [key for key in sorted(set(want) | set(got)) if want.get(key) != got.get(key)]
    for key in diff:
        print("%s:\n  recorded %s\n  now      %s" % (key, want.get(key), got.get(key)))
    assert not diff, "%d parts of the monitor surface moved (see above); a deliberate change rewrites %s" % (len(diff), GOLDEN)


def test_attach_takes_what_set_monitor_takes():
    from trex_gym import monitor, vec_env
    a = list(inspect.signature(monitor.attach).parameters.values())[1:]
    b = list(inspect.signature(vec_env.TrexVecEnv._set_monitor).parameters.values())[1:]
    assert [(p.name, p.default) for p in a] == [(p.name, p.default) for p in b]


def test_the_env_class_gained_one_private_method_and_nothing_public():
    from trex_gym import vec_env
    assert [a for a in vars(vec_env.TrexVecEnv) if "monitor" in a] == ["_set_monitor"]


def test_the_symbols_are_the_header_s():
    """every function include/trex_monitor.h declares is in the signature table, with as many arguments, and none besides; the
    summary's indices are the header's"""
    from trex_gym import monitor_capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "trex_monitor.h")).read(), flags=re.S)
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\bint\s+(trex_batch_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(monitor_capi.MONITOR_SYMBOLS)
    for name, (_, argtypes) in monitor_capi._MONITOR_API.items():
        assert len(argtypes) == declared[name], name
    defines = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+TREX_MON_(\w+)\s+(\d+)", text)}
    for k in ("N", "RET_MEAN", "RET_MIN", "RET_MAX", "LEN_MEAN", "LEN_MIN", "LEN_MAX", "WIN_REASON", "TOTAL", "BY_REASON", "T", "SUMMARY"):
        assert defines[k] == getattr(monitor_capi, k), k
    assert (defines["MAXWINDOW"], defines["MAXCOLS"]) == (monitor_capi.MAX_WINDOW, monitor_capi.MAX_COLS)


def test_the_reference_uses_the_header_s_indices():
    import monitor_ref as MR
    from trex_gym import monitor_capi as M
    for k in ("N", "RET_MEAN", "RET_MIN", "RET_MAX", "LEN_MEAN", "LEN_MIN", "LEN_MAX", "WIN_REASON", "TOTAL", "BY_REASON", "T", "SUMMARY"):
        assert getattr(MR, k) == getattr(M, k), k
    assert (MR.MAXWINDOW, MR.MAXCOLS) == (M.MAX_WINDOW, M.MAX_COLS)


def test_merged_summaries_weigh_every_rank_by_its_window():
    from trex_gym import monitor, monitor_capi as M
    nan = float("nan")
    a = [4, 2.0, 1.0, 3.0, 10.0, 8.0, 12.0, 3, 1, 0, 0, 40, 30, 10, 0, 0, 7, 0.5]
    b = [1, 7.0, 7.0, 7.0, 5.0, 5.0, 5.0, 0, 0, 1, 1, 1, 0, 0, 1, 1, 7, -2.0]
    empty = [0, nan, nan, nan, nan, nan, nan, 0, 0, 0, 0, 0, 0, 0, 0, 0, 7, nan]
    m = monitor.merge_summaries([a, b, empty])
    assert m[M.N] == 5 and m[M.RET_MEAN] == 3.0 and m[M.LEN_MEAN] == 9.0 and m[M.SUMMARY] == 0.0
    assert (m[M.RET_MIN], m[M.RET_MAX], m[M.LEN_MIN], m[M.LEN_MAX]) == (1.0, 7.0, 5.0, 12.0)
    assert m[M.WIN_REASON:M.WIN_REASON + 4] == [3, 1, 1, 1] and m[M.TOTAL] == 41 and m[M.BY_REASON:M.BY_REASON + 4] == [30, 10, 1, 1]
    stats = monitor.stats_from_summary(m, ["alive"])
    assert stats["end_reasons"] == dict(limit=0.6, head=0.2, tilt=0.2, clearance=0.2) and stats["terms"] == {"alive": 0.0}
    none = monitor.stats_from_summary(monitor.merge_summaries([empty, empty]))
    assert none["window_episodes"] == 0 and none["eprewmean"] != none["eprewmean"]


if __name__ == "__main__":
    import sys
    sys.path[:0] = [ROOT, os.path.join(ROOT, "trex-gym_amd")]
    with open(GOLDEN, "w") as f:
        json.dump(surface(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", GOLDEN)
