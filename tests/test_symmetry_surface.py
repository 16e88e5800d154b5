"""The C surface of the mirror maps on the CPU: every function include/trex_symmetry.h declares is in the signature table of
trex_gym/symmetry_capi.py with as many arguments, and none besides; the built library exports each; the header stands alone; the
constants agree; the Python surface is there."""
import inspect
import os
import re

from conftest import ROOT


def _header():
    raw = open(os.path.join(ROOT, "include", "trex_symmetry.h")).read()
    return raw, re.sub(r"/\*.*?\*/", "", raw, flags=re.S)


def test_the_symbols_are_the_header_s():
    from trex_gym import symmetry_capi as S
    raw, text = _header()
    declared = {m.group(1): len(m.group(2).split(",")) for m in re.finditer(r"\b(?:int|void)\s+(trex_\w+)\s*\(([^)]*)\)\s*;", text)}
    assert sorted(declared) == sorted(S.SYMMETRY_SYMBOLS) and len(declared) == 10
    for name, (_, argtypes) in S._SYMMETRY_API.items():
        assert len(argtypes) == declared[name], name
        assert hasattr(S.lib, name), name
    assert re.findall(r'#include\s+"([^"]+)"', raw) == [] and re.findall(r"#include\s+<([^>]+)>", raw) == ["stdint.h"]
    # the trainer's own header declares none of them (its symbol list is pinned by tests/test_capi_host.py)
    policy_h = open(os.path.join(ROOT, "include", "trex_policy.h")).read()
    assert not any(name + "(" in policy_h.replace(" (", "(") for name in declared)


def test_the_constants_are_the_header_s():
    from trex_gym import symmetry_capi as S
    import symmetry_ref as R
    _, text = _header()
    assert int(re.search(r"#define\s+TREX_MIRROR_MAXWIDTH\s+(\d+)", text).group(1)) == S.MAX_WIDTH == R.MAXWIDTH == 517
    limits = open(os.path.join(ROOT, "trex-gym_amd", "csrc", "symmetry_limits.h")).read()
    tile = int(re.search(r"#define\s+TREX_MIRROR_TILE_FLOATS\s+(\d+)", limits).group(1))
    assert tile >= S.MAX_WIDTH                          # a tile holds at least one row of the widest table
    assert tuple(S.RESIDUALS) == tuple(R.RESIDUALS) and len(S.RESIDUALS) == 5
    batch_h = open(os.path.join(ROOT, "include", "trex_batch.h")).read()
    kinds = dict(re.findall(r"#define\s+TREX_OBS_(\w+)\s+(\d+)", batch_h))
    for name in ("PROJECTED_GRAVITY", "BASE_LINEAR_VELOCITY", "BASE_ANGULAR_VELOCITY", "BASE_HEIGHT", "POINT_POSITION", "POINT_VELOCITY",
                 "POINT_HEIGHT", "CONTACT_FORCE", "PREV_ACTION", "EXTERNAL"):
        assert int(kinds[name]) == getattr(R, name), name


def test_the_python_surface():
    from trex_gym import symmetry
    assert {"symmetry", "mirror", "sym_coef"} <= set(inspect.signature(symmetry.MirrorPPO.__init__).parameters)
    assert callable(symmetry.symmetrize_theta) and callable(symmetry.Mirror.symmetric_action)
    assert [a for a in ("rows", "actions", "command", "state", "tables") if not callable(getattr(symmetry.Mirror, a, None))] == []
