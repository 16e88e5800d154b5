"""The packed rows of the device model (csrc/device_model.h: tree_pack, child_pack, hull_range, chunk_row, chunk_box), on the CPU
and under the sanitizers: fill_device_model built with csrc/model.cpp into tests/host/packed_model_harness.cpp by g++
-fsanitize=address,undefined (the flags of tests/test_host_tables.py; no HIP, nothing loaded into Python), one child process per
model. The step kernel fetches these rows once per substep, every lane at its own index and with no select in front of the load;
until then it formed the same words per lane from `parent`, `depth`, `child`, `hull_start`, `cm_pack` and the chunk tables. That
derivation is restated here, lane by lane, from the tables the same run prints (tests/test_host_tables.py pins those against the
oracle's model), and every packed word must equal it exactly - floats included: they are copies."""
import os
import subprocess

import numpy as np
import pytest

import synthetic_models as SM
from conftest import ASSET_URDF, ROOT

CSRC = os.path.join(ROOT, "trex-gym_amd", "csrc")
NONE = 0xFFFFFFFF      # child_pack of a body without a moving child, and of a lane that is no body


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_packed") / "packed_model_harness")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "packed_model_harness.cpp"), os.path.join(CSRC, "host_tables.cpp"),
                           os.path.join(CSRC, "model.cpp")])
    return exe


def tables(exe, urdf):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, urdf], env=env, capture_output=True, text=True, timeout=120)
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    t = {}
    for line in r.stdout.splitlines():
        name, *vals = line.split()
        t[name] = np.array(vals, np.float64) if name in ("chunk_c", "chunk_h", "chunk_box") else np.array([int(v) for v in vals], np.int64)
    return t


def check_packed(t):
    """every packed word against what the kernel derived per lane; -> (nb, children per body lane)"""
    nb, nchunk, TL, MAXCH, NO_DEPTH, o_range, o_row, o_box = t["scalars"].tolist()
    assert (TL, MAXCH, NO_DEPTH) == (32, 4, 255) and 1 <= nb <= TL and 0 <= nchunk <= TL
    assert o_range % 8 == 0 and o_row % 16 == 0 and o_box % 16 == 0     # fetched as aligned 2- and 4-word loads
    parent, depth, child = t["parent"], t["depth"], t["child"].reshape(MAXCH, TL)
    hs, cm = t["hull_start"], t["cm_pack"]
    hr, row, box = t["hull_range"].reshape(TL, 2), t["chunk_row"].reshape(TL, 4), t["chunk_box"].reshape(TL, 8)
    cc, ch = t["chunk_c"].reshape(3, TL), t["chunk_h"].reshape(3, TL)
    kids = []
    for l in range(TL):
        is_body = l < nb
        # the substep's top: parent = is_body ? parent[bl] : 0; psrc = max(parent, 0); depth = is_body ? depth[bl] : -1; the
        # record word psrc + 256 * (depth < 0 ? 255 : depth)
        p = int(parent[l]) if is_body else 0
        d = int(depth[l]) if is_body else -1
        assert t["tree_pack"][l] == max(p, 0) | ((NO_DEPTH if d < 0 else d) << 8), l
        # FK: ch4 |= (c < 0 ? 255 : c) << 8 k with c = is_body ? child[k][bl] : -1
        ch4 = 0
        for k in range(MAXCH):
            c = int(child[k, l]) if is_body else -1
            ch4 |= (255 if c < 0 else c) << (8 * k)
        assert t["child_pack"][l] == ch4, l
        kids.append(sum(1 for k in range(MAXCH) if (ch4 >> (8 * k)) & 255 != 255))
        # contact generation: hull_start[is_body ? lt : nb], hull_start[is_body ? lt + 1 : nb]
        assert hr[l].tolist() == [hs[l if is_body else nb], hs[l + 1 if is_body else nb]], l
        # broad phase: chunk_body, chunk_v0, is_chunk ? chunk_v1 : 0; the table entry cbody | cm_pack[cbody] << 8, hull_start[cbody]
        if l < nchunk:
            cb = int(t["chunk_body"][l])
            assert 0 <= cb < nb
            assert row[l].tolist() == [cb | (int(cm[cb]) << 8), t["chunk_v0"][l], t["chunk_v1"][l], hs[cb]], l
            assert row[l][0] & 255 == cb and row[l][0] >> 8 == cm[cb]
        else:
            assert row[l].tolist() == [0, 0, 0, 0] and t["chunk_body"][l] == 0 and t["chunk_v0"][l] == 0, l
        assert box[l].tolist() == [cc[0, l], cc[1, l], cc[2, l], 0.0, ch[0, l], ch[1, l], ch[2, l], 0.0], l
    return nb, kids


def assert_defaults_beyond(t, nb):
    """the lanes >= nb carry what the kernel gave a lane that is no body: parent 0, no depth, no child, the empty hull range"""
    assert nb < 32
    end = t["hull_start"][nb]
    for l in range(nb, 32):
        assert t["tree_pack"][l] == 255 << 8 and t["child_pack"][l] == NONE
        assert t["hull_range"].reshape(32, 2)[l].tolist() == [end, end]


def test_packed_rows_trex(harness):
    t = tables(harness, ASSET_URDF)
    nb, kids = check_packed(t)
    assert nb == 26
    assert_defaults_beyond(t, nb)
    assert min(kids[:nb]) == 0 and max(kids[:nb]) >= 2                   # leaves, and the pelvis with more than one child
    assert t["tree_pack"][0] == 0                                        # the base: parent -1 reads as lane 0, depth 0


@pytest.mark.parametrize("name", sorted(SM.MODELS))
def test_packed_rows_generated(harness, tmp_path, name):
    path, props, m = SM.compile_both(name, tmp_path / name)
    t = tables(harness, path)
    nb, kids = check_packed(t)
    assert nb == m["nb"]
    assert_defaults_beyond(t, nb)
    depths = t["tree_pack"][:nb] >> 8
    assert depths.max() == props["depth"]
    if name == "deep_chain":
        assert depths.max() == 6
    if name == "bushy":
        # four moving children (MAXCH) on two bodies, at the depths the generator states; the six welded links are merged into their
        # hosts, so no packed word names them; and bodies with no child at all
        full = [b for b in range(nb) if kids[b] == 4]
        assert len(full) == len(props["four_children"]) == 2 and sorted(depths[full].tolist()) == props["four_children_depths"]
        for b in full:
            assert sorted((int(t["child_pack"][b]) >> (8 * k)) & 255 for k in range(4)) == [c for c in range(1, nb) if m["parent"][c] == b]
        assert nb == props["nb"] and len(m["link_names"]) == nb + props["merged_links"]
        assert kids[:nb].count(0) >= len(props["hull_less"])
        assert (t["child_pack"][[b for b in range(nb) if kids[b] == 0]] == NONE).all()
