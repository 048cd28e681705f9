#!/usr/bin/env python3
"""Writer of tests/golden/batch_plan_table.json: which of their two kernels dff_msm_dirichlet_solve, dff_sym_eig_topk and
dff_msm_propagate launch, and on which problems, for every debug path and the state counts that their selection rules name
(tests/test_msm_batch_plan.py pins the host-only plan, dff_debug_msm_batch_plan, to it).

The three rules below are a statement of the batched solvers' host code (csrc/dff_analysis.hip then, csrc/dff_an_markov.hip now) as it was when each call still carried a selection of its own:
one function per call, written from that code line by line, not from the function that replaced them.  No GPU, no library:
python tests/golden/make_batch_plan_table.py [out.json]

File layout: `limits` (call -> the LDS limit the table was made with, in the call's own size measure: K_p, or the interior count
for the Dirichlet solver), `kmax` (the Kmax of every case) and `records`, one per (call, knob, ks): {"call", "knob", "ks",
"launches": [lds, other]} with a launch null (not launched) or [path, lo, hi, sizing argument] -- the sizing argument is what
the launch's LDS bytes are computed for, null where they do not depend on the problems -- or {"call", "knob", "ks", "refused":
message}."""
import json
import os
import sys

LIMITS = {"dirichlet": 128, "eig": 176, "propagate": 120}
KNOBS = {"dirichlet": (0, 1, 2, 3, 4), "eig": (0, 1, 2), "propagate": (0, 1, 2)}
WHAT = {"dirichlet": "msm_dirichlet_solve", "eig": "sym_eig_topk", "propagate": "msm_propagate"}
KMAX = 1024
INT_MAX = 0x7FFFFFFF


class Refused(Exception):
    pass


def check_ks(what, ks, forced_max):
    """the loop over ks[p] that every call ran: the range, then the forced LDS path's limit, problem by problem"""
    for p, k in enumerate(ks):
        if k < 1 or k > KMAX:
            raise Refused(f"{what}: problem {p} has {k} states, must be 1..Kmax = {KMAX}")
        if forced_max is not None and k > forced_max:
            raise Refused(f"{what}: problem {p} has {k} states, the forced LDS path takes at most {forced_max}")
    return min(ks), max(ks)


def dirichlet(knob, ks):
    L = LIMITS["dirichlet"]
    path = 2 if knob > 2 else knob                   # 3 and 4: the blocked path with a named trailing update
    _, kmax_live = check_ks(WHAT["dirichlet"], ks, L + 1 if path == 1 else None)
    lds = other = None
    if path != 2:                                    # interior counts 0 .. the limit (all of them when forced)
        lds = [1, 0, INT_MAX if path == 1 else L, min(kmax_live - 1, L)]
    if path == 2 or (path == 0 and kmax_live > L):   # the blocked kernel's LDS is one fixed size
        other = [2, 0 if path == 2 else L + 1, INT_MAX, None]
    return [lds, other]


def by_state_count(call):
    def rule(knob, ks):
        L = LIMITS[call]
        kmin_live, kmax_live = check_ks(WHAT[call], ks, L if knob == 1 else None)
        lds = other = None
        if knob == 1 or (knob == 0 and kmin_live <= L):
            lds = [1, 1, L, min(kmax_live, L)]
        if knob == 2 or (knob == 0 and kmax_live > L):
            other = [2, 1 if knob == 2 else L + 1, KMAX, kmax_live]
        return [lds, other]
    return rule


RULES = {"dirichlet": dirichlet, "eig": by_state_count("eig"), "propagate": by_state_count("propagate")}


def cases(call):
    """the state counts the rules name; `top` is the largest K_p the LDS path can take, `above` the first it cannot"""
    L = LIMITS[call]
    off = 1 if call == "dirichlet" else 0            # an interior count is at most K_p - 1
    top, above = L + off, L + off + 1
    out = [[1], [L], [L + 1]] + ([[L + 2]] if call == "dirichlet" else []) + [[1024]]
    out += [[2, top // 2, top], [above, 300, 1024], [top, above], [1024, above, 3]]
    return out


def main(argv):
    records = []
    for call in ("dirichlet", "eig", "propagate"):
        for knob in KNOBS[call]:
            for ks in cases(call):
                rec = {"call": call, "knob": knob, "ks": ks}
                try:
                    rec["launches"] = RULES[call](knob, ks)
                except Refused as e:
                    rec["refused"] = str(e)
                records.append(rec)
    out = argv[1] if len(argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "batch_plan_table.json")
    with open(out, "w") as f:
        f.write('{"limits": %s, "kmax": %d, "records": [\n' % (json.dumps(LIMITS), KMAX))
        f.write(",\n".join(json.dumps(r) for r in records))
        f.write("\n]}\n")
    print(f"{len(records)} records -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
