#!/usr/bin/env python3
"""Is the device code of the step kernels the same in two source trees?  No GPU needed.

    python scripts/compare_step_kernels.py --parent REV [--units A,B] [--out profiles/NAME.txt] [--keep DIR] [--expect-different NAME]...

Compiles the kernel units of git revision REV and of the working tree - trex_step.hip, trex_step_act.hip, dynamics.hip and
batch_util.hip, those a side has, or the units named with --units (the trainer's: --units policy_step,ppo_learner) - to gfx950 assembly with the Makefile's flags (hipcc --cuda-device-only -S), as the product build and as the stamped build (-DTREX_STAMPS=1), and
pairs every kernel of one side with its counterpart of the other: a step kernel by WHAT it is - (form, WARM, EXT, SENS,
ACT), read off its demangled name under either naming, the wrapper families `trex_step{,_pair,_many}{,_warm,_ext,_sens,
_act}_kernel` / `trex_reset_sens_kernel` or the one template `trex_step_variant_kernel<FORM, WARM, EXT, SENS, ACT>` -, a
utility kernel by its name, whichever unit it lives in (a move between units is shown, `trex_step -> batch_util`, and is no
difference; a step kernel has to stay in its unit). A pair is IDENTICAL when the instruction text from the kernel's label to its .Lfunc_end and
its .amdhsa_* descriptor block are the same lines, after the kernel's own symbol and the function index inside local
labels (.LBB<n>_, .Lfunc_end<n>) are normalised and the directives that place a kernel in a section are left out. Exit
status 0 only if every kernel has a partner, every pair is identical - but for the utility kernels named with --expect-different,
which are listed with their figures on both sides and must not use scratch - and no kernel of the product build has a private
segment (scratch; the stamped diagnostic build has some, on both sides alike). With --units only the product build is compared
(TREX_STAMPS is the step kernels' switch) and scratch is listed, not judged: identical is the whole question there."""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "trex-gym_amd/csrc"
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=fast", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
UNITS = ["trex_step", "trex_step_act", "dynamics", "batch_util"]   # those of them a side has
BUILDS = [("product", []), ("stamped", ["-DTREX_STAMPS=1"])]
FORMS = {0: "single", 1: "many", 2: "reset", 3: "debug", 4: "pair"}   # FORM of trex_step_variant_kernel (trex_step.hip)


def what(name):
    """demangled kernel name -> (form, WARM, EXT, SENS, ACT) of a step kernel, or the bare name of a utility kernel"""
    m = re.match(r"(?:void )?(\w+?)(?:<([^>]*)>)?\(", name)
    base, targs = m.group(1), [a.strip() for a in (m.group(2) or "").split(",") if a.strip()]
    b = [a == "true" for a in targs]
    if base == "trex_step_variant_kernel":
        return (FORMS[int(re.sub(r"\D", "", targs[0]))],) + tuple(b[1:5])
    if base == "trex_reset_sens_kernel":
        return ("reset", b[0], False, True, False)
    m = re.fullmatch(r"trex_step(_pair|_many)?(_warm|_ext|_sens|_act)?_kernel", base)
    if not m:
        return base + ("<%s>" % ", ".join(targs) if targs else "")
    form, feat = (m.group(1) or "_single")[1:], m.group(2)
    if feat is None:       # <RESET, DEBUG> on the single-env kernel
        return ("reset" if b[:1] == [True] else "debug" if b[1:2] == [True] else form, False, False, False, False)
    if feat == "_warm":    # <RESET> on the single-env kernel
        return ("reset" if b[:1] == [True] else form, True, False, False, False)
    if feat == "_ext":     # <WARM>
        return (form, b[0], True, False, False)
    if feat == "_sens":    # <WARM, EXT>
        return (form, b[0], b[1], True, False)
    return (form, b[0], b[1], b[2], True)   # _act: <WARM, EXT, SENS>


def kernels(asm_path):
    """{what: {"name", "text", "desc", figures}} of one assembly file"""
    lines = open(asm_path).read().split("\n")
    syms = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    plain = subprocess.run(["c++filt"] + syms, capture_output=True, text=True, check=True).stdout.split("\n") if syms else []
    start = {l.split(":")[0]: i for i, l in enumerate(lines) if l.startswith("_Z") and l.split(":")[0] in set(syms)}
    out = {}
    for sym, name in zip(syms, plain):
        name = name.replace("(anonymous namespace)::", "")
        i = start[sym]
        j = next(k for k in range(i, len(lines)) if re.fullmatch(r"\.Lfunc_end\d+:", lines[k]))
        d0 = next(k for k in range(i, j) if lines[k].strip().startswith(".amdhsa_kernel "))
        d1 = next(k for k in range(d0, j) if lines[k].strip() == ".end_amdhsa_kernel")
        info = "\n".join(lines[j:j + 40])

        def norm(ls):   # (and the section a kernel is placed in - .text or a comdat group of its own - is linkage, not code)
            t = "\n".join(l for l in ls if l.split()[:1] not in ([".text"], [".section"])).replace(sym, "KERNEL")
            t = re.sub(r"[ \t]*;", " ;", t)                                    # (comment columns move with the length of a name)
            return re.sub(r"(\.Lfunc_end|\.Lfunc_begin|BB)\d+", r"\1", t)       # .LBB<n>_k, and BB<n>_k inside comments

        def fig(pat):
            return int(re.search(pat, info).group(1))

        k = what(name)
        assert k not in out, "two kernels are the same thing: %s" % (k,)
        out[k] = {"name": name, "text": norm(lines[i:d0] + lines[d1 + 1:j + 1]), "desc": norm(lines[d0:d1 + 1]),
                  "vgprs": fig(r"; NumVgprs: (\d+)"), "sgprs": fig(r"; TotalNumSgprs: (\d+)"), "scratch": fig(r"; ScratchSize: (\d+)"),
                  "lds": fig(r"; LDSByteSize: (\d+)"), "private": int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", "\n".join(lines[d0:d1])).group(1))}
    return out


def compile_tree(csrc, dest, units, builds):
    jobs = []
    for unit in units:
        if not os.path.exists(os.path.join(csrc, unit + ".hip")):
            continue
        for tag, extra in builds:
            out = os.path.join(dest, "%s.%s.s" % (unit, tag))
            jobs.append((out, [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + extra + ["-o", out, unit + ".hip"]))
    with concurrent.futures.ThreadPoolExecutor(len(jobs)) as ex:
        for r in ex.map(lambda j: subprocess.run(j[1], cwd=csrc, capture_output=True, text=True), jobs):
            if r.returncode:
                sys.exit(r.stderr)


def label(k):
    return k if isinstance(k, str) else "%-6s %s" % (k[0], " ".join(n if on else "-" * len(n) for n, on in zip(("WARM", "EXT", "SENS", "ACT"), k[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="git revision to compare the working tree with")
    ap.add_argument("--out", help="write the report here as well")
    ap.add_argument("--keep", help="directory for the assembly files (kept; files already there are reused)")
    ap.add_argument("--expect-different", action="append", default=[], metavar="NAME",
                    help="a utility kernel that is rewritten on purpose: DIFFERENT is accepted for it, scratch is not (repeatable)")
    ap.add_argument("--units", help="comma-separated kernel units to compare instead of %s" % ",".join(UNITS))
    a = ap.parse_args()
    units = a.units.split(",") if a.units else UNITS
    builds = BUILDS[:1] if a.units else BUILDS
    work = a.keep or tempfile.mkdtemp(prefix="step_kernels_")
    sides = {}
    for side in ("parent", "tree"):
        dest = os.path.join(work, side)
        if not os.path.isdir(dest):
            os.makedirs(dest)
            csrc = os.path.join(ROOT, CSRC)
            if side == "parent":
                tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, CSRC, "include"], capture_output=True, check=True).stdout
                subprocess.run(["tar", "-x", "-C", dest], input=tar, check=True)
                csrc = os.path.join(dest, CSRC)
            compile_tree(csrc, dest, units, builds)
        sides[side] = dest
    rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", a.parent], capture_output=True, text=True, check=True).stdout.strip()
    rep = ["kernels of %s: the working tree against %s: device assembly, kernel by kernel (scripts/compare_step_kernels.py)" % (", ".join(u + ".hip" for u in units), rev),
           "hipcc " + " ".join(FLAGS), ""]
    bad = 0
    for tag, extra in builds:
        old, new = {}, {}
        for unit in units:
            for side, dst in (("parent", old), ("tree", new)):
                asm = os.path.join(sides[side], "%s.%s.s" % (unit, tag))
                if not os.path.exists(asm):
                    continue
                ks = kernels(asm)
                assert not set(ks) & set(dst), "a kernel in both translation units"
                for k in ks.values():
                    k["unit"] = unit
                dst.update(ks)
        steps = sorted(k for k in set(old) | set(new) if not isinstance(k, str))
        utils = sorted(k for k in set(old) | set(new) if isinstance(k, str))
        rep.append("== %s build%s: %d step kernels, %d utility kernels (parent: %d, %d)" % (
            tag, " (%s)" % " ".join(extra) if extra else "", sum(not isinstance(k, str) for k in new), sum(isinstance(k, str) for k in new),
            sum(not isinstance(k, str) for k in old), sum(isinstance(k, str) for k in old)))
        rep.append("%-34s %-10s %5s %5s %8s %7s  %-26s parent kernel -> kernel" % ("what", "result", "VGPRs", "SGPRs", "scratch", "LDS", "unit"))
        for k in steps + utils:
            o, n = old.get(k), new.get(k)
            if not o or not n:
                res = "NO PARENT" if n else "MISSING"
            else:
                same = o["text"] == n["text"] and o["desc"] == n["desc"] and all(o[f] == n[f] for f in ("vgprs", "sgprs", "scratch", "private", "lds"))
                res = "identical" if same and (isinstance(k, str) or o["unit"] == n["unit"]) else "DIFFERENT"
            x = n or o
            scratch_free = all(y["scratch"] == 0 and y["private"] == 0 for y in (o, n) if y)
            expected = res == "DIFFERENT" and k in a.expect_different
            bad += (res != "identical" and not expected) or ((tag == "product" or expected) and not scratch_free and not a.units)
            unit = x["unit"] if not o or not n or o["unit"] == n["unit"] else "%s -> %s" % (o["unit"], n["unit"])
            line = "%-34s %-10s %5d %5d %8d %7d  %-26s %s -> %s" % (label(k), res, x["vgprs"], x["sgprs"], max(x["scratch"], x["private"]),
                                                                  x["lds"], unit, o["name"].split("(")[0] if o else "-", n["name"].split("(")[0] if n else "-")
            if res == "DIFFERENT":   # the figures of both sides
                line += "   [parent: %d VGPRs, %d SGPRs, scratch %d, LDS %d%s]" % (o["vgprs"], o["sgprs"], max(o["scratch"], o["private"]), o["lds"],
                                                                                 "; expected (--expect-different)" if expected else "")
            rep.append(line)
        rep.append("")
    rep.append("RESULT: %s" % ("every pair identical%s%s" % (
        " but the expected %s" % ", ".join(a.expect_different) if a.expect_different else "",
        "" if a.units else ", no kernel of the product build with a private segment") if not bad else "%d kernel(s) differ, lack a partner or use scratch" % bad))
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
