"""States and thresholds for the tests of fall termination (include/trex_batch.h: trex_batch_set_termination). Everything is
generated from seeds and qualified by the f64 reference alone (tests/termination_ref.py): tests/test_termination_cases_host.py
asserts on the CPU that the sample is what it claims, tests/test_gpu_termination.py feeds the same arrays to the kernel. A helper,
not a conftest.

States, per collision model:
  hulls       every accepted fallen state of episode_cases' groups `hulls` and `hulls_domain` (the latter with its mass scales), then
              the start state at rest and the 33 landing / airborne states of state_sets.case_states;
  primitives  every accepted fallen state of episode_cases' group `primitives`, then the start state.
Thresholds, per collision model, from the reference's values on these states alone: a head height, a tilt (as its cosine) and a
least clearance of ONE watched body, each the midpoint of a gap of at least MIN_GAP between two neighbours of the sorted values -
so that every state sits MIN_GAP / 2 >= 1e-3 away from it (m; cos tilt: 1). Which gaps: the first, in the order of `search`, for
which each reason fires alone in >= 5 states, two at once in >= 5 and none in at least a third."""
import numpy as np

import episode_cases as ec
import feature_cases as fc
import termination_ref as TR
from state_sets import case_states

MIN_GAP = 2.5e-3
CLEAR = 1e-3          # what the host test asserts: every state at least this far from every threshold
# (the fallen states crowd the middle of every value's range: gaps of MIN_GAP are found in the tails, so the search starts there
# from the largest fraction that may still leave a third of the states alone)
FRACTIONS = (0.3, 0.2, 0.15, 0.1, 0.07, 0.05, 0.03, 0.02, 0.01)
WATCH = ("link_cranium", "link_vertebrae_sacral", "link_vertebra_caudal_24", "link_vertebra_caudal_02")

_CACHE = {}


def states(collision):
    """-> (built, [dict(state f32 [63], mass_scale f32 [nb] or None, origin)])"""
    key = ("states", collision)
    if key in _CACHE:
        return _CACHE[key]
    out = []
    if collision == "primitives":
        g = ec.group("primitives")
        b = g["built"]
        out += [dict(state=c["state"], mass_scale=None, origin="primitives " + c["origin"]) for c in g["cases"]]
    else:
        g = ec.group("hulls")
        b = g["built"]
        out += [dict(state=c["state"], mass_scale=None, origin="hulls " + c["origin"]) for c in g["cases"]]
        out += [dict(state=c["state"], mass_scale=c["mass_scale"], origin="hulls_domain " + c["origin"])
                for c in ec.group("hulls_domain")["cases"]]
    out.append(dict(state=fc.start_state(b.om).astype(np.float32), mass_scale=None, origin="start"))
    if collision != "primitives":
        for k, (s, ms) in enumerate(case_states(b.o64, b.om, 33)):
            out.append(dict(state=s.astype(np.float32), mass_scale=None if ms is None else ms.astype(np.float32),
                            origin="case_states %d" % k))
    _CACHE[key] = (b, out)
    return _CACHE[key]


def reference(collision):
    """the reference's evaluation of every state: list of termination_ref.evaluate dicts"""
    key = ("ref", collision)
    if key not in _CACHE:
        b, cs = states(collision)
        _CACHE[key] = [TR.evaluate(b.o64, b.om, c["state"].astype(np.float64), c["mass_scale"]) for c in cs]
    return _CACHE[key]


def gap_midpoint(vals, frac):
    """midpoint of the first gap >= MIN_GAP between neighbours of the sorted finite values, from the quantile `frac` upwards"""
    v = np.sort(np.asarray(vals, np.float64)[np.isfinite(vals)])
    for k in range(int(frac * len(v)), len(v) - 1):
        if v[k + 1] - v[k] >= MIN_GAP:
            return 0.5 * (v[k] + v[k + 1])
    return None


def counts(reasons):
    r = np.asarray(reasons)
    return dict(head=int((r == TR.HEAD).sum()), tilt=int((r == TR.TILT).sum()), clearance=int((r == TR.CLEARANCE).sum()),
                two=int(np.isin(r, (3, 5, 6)).sum()), none=int((r == 0).sum()), n=len(r))


def qualifies(c):
    return min(c["head"], c["tilt"], c["clearance"], c["two"]) >= 5 and 3 * c["none"] >= c["n"]


def search(collision):
    """-> dict(head_height, cos_tilt, max_tilt, body, link, clear, clear_min [nb] with NaN = not watched, reasons [cases],
    values [cases, 3]) - the first threshold set that qualifies, None if there is none"""
    key = ("thr", collision)
    if key in _CACHE:
        return _CACHE[key]
    b, _ = states(collision)
    ref = reference(collision)
    head = np.array([e["head"] for e in ref])
    cost = np.array([e["cos_tilt"] for e in ref])
    found = None
    for link in WATCH:
        if link not in list(b.om["link_names"]):
            continue
        body =int(b.om["link_body"][list(b.om["link_names"]).index(link)])
        clr = np.array([e["clearance"][body] for e in ref])
        for fc_ in FRACTIONS:
            cm = gap_midpoint(clr, fc_)
            for fh in FRACTIONS:
                hh = gap_midpoint(head, fh)
                for ft in FRACTIONS:
                    ct = gap_midpoint(cost, ft)
                    if None in (cm, hh, ct) or not -1.0 < ct < 1.0:
                        continue
                    quick = (head < hh) * TR.HEAD + (cost < ct) * TR.TILT + (clr - cm < 0) * TR.CLEARANCE
                    if not qualifies(counts(quick)):
                        continue
                    clear_min = np.full(b.nb, np.nan)
                    clear_min[body] = cm
                    tilt = float(np.arccos(ct))
                    vals = np.array([TR.values(e, clear_min) for e in ref])
                    reasons = np.array([TR.reason(v, hh, tilt) for v in vals])
                    if qualifies(counts(reasons)):
                        found = dict(head_height=float(hh), cos_tilt=float(ct), max_tilt=tilt, body=body, link=link, clear=float(cm),
                                     clear_min=clear_min, reasons=reasons, values=vals)
                        break
                if found:
                    break
            if found:
                break
        if found:
            break
    _CACHE[key] = found
    return found


def sample(collision, n=67):
    """indices of n states spread over the list, the last ones (start, landing, airborne) included"""
    total = len(states(collision)[1])
    return np.unique(np.round(np.linspace(0, total - 1, n)).astype(int))
