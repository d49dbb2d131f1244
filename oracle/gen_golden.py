#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — regenerate tests/golden/ from the REAL reference.

Runs oracle/_ref/ref_harness (christang/alignment-algos compiled in place from
/root/reference by oracle/Makefile) on seeded synthetic inputs and stores its outputs:

  tests/golden/aa_cases.json   metadata, scores (as uint32 bit patterns), pair lists, gapped strings
  tests/golden/aa_cases.npz    full score / pointer / similarity matrices of the small cases
  tests/golden/profile_cases.*        the profile path at its default parameters (oracle/_ref/ref_profile)
  tests/golden/profile_param_cases.*  the profile path off them; `gen_golden.py profile_params` rewrites these two alone,
                                      byte for byte
  tests/golden/enum_modes.json        CW / UCW sets in the one-sided align types 0 and 2 (cases of tests/enum_mode_cases.py);
                                      `gen_golden.py enum_modes` rewrites this file alone
  tests/golden/enum_chain.json        two enumerations in a row on one AlignmentSet (chains of tests/enum_pool_cases.py);
                                      `gen_golden.py enum_chain` rewrites this file alone

Only this container has /root/reference; the fixtures are what travels.  Inputs are
regenerated from seeds by aln_amd.synth (std::mt19937-compatible), but the sequences are
also stored so the fixtures are self-contained.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))
import orc  # noqa: E402  (only for make_subopt_regions)
import refrun  # noqa: E402
from aln_amd.synth import MT19937, homolog_pair, random_pair, residues  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def bits(x):
    return int(np.float32(x).view(np.uint32))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def ali_json(a):
    d = {"score": bits(a["score"]), "identity": bits(a["identity"]), "uid": a["uid"],
         "pairs": a["pairs"].reshape(-1).tolist(), "annot": a["annot"]}
    if "qstr" in a:
        d["qstr"] = a["qstr"]
    return d


def set_json(s, full_limit=None):
    """Alignments past `full_limit` keep score/uid and sha256 digests of their pair list and query line."""
    alis = []
    for k, a in enumerate(s["alis"]):
        if full_limit is None or k < full_limit:
            alis.append(ali_json(a))
        else:
            alis.append({"score": bits(a["score"]), "identity": bits(a["identity"]), "uid": a["uid"],
                         "pairs_sha": sha(a["pairs"].astype(np.int32)),
                         "qstr_sha": hashlib.sha256(a.get("qstr", "").encode()).hexdigest()})
    d = {"n": s["n"], "alis": alis}
    if "tstr" in s:
        d["tstr"] = s["tstr"]
    return d


def main():
    if not refrun.available():
        raise SystemExit("oracle/_ref/ref_harness missing: run `make -C oracle` where /root/reference exists")
    cases = []
    arrays = {}

    def add(name, q, t, mode, gi, ge, direction, ops, full, extra=None, sets_full=False):
        r = refrun.run_aa(q, t, mode, gi, ge, direction, ops=["dump"] + list(ops))
        c = {"name": name, "q": q, "t": t, "mode": mode, "gi": gi, "ge": ge, "dir": direction}
        if extra:
            c.update(extra)
        if "throw" in r:
            c["throw"] = r["throw"]
        if "dim" in r:
            c["sha"] = {"H": sha(r["H"]), "PQ": sha(r["PQ"]), "PT": sha(r["PT"])}
            c["corner"] = bits(r["H"][-1, -1])
            c["origin"] = bits(r["H"][0, 0])
            if full:
                for k in ("H", "PQ", "PT", "S"):
                    arrays["%s/%s" % (name, k)] = r[k]
        c["sets"] = {k: set_json(v, None if (full or sets_full) else 6) for k, v in r["sets"].items()}
        cases.append(c)

    # A. known answers of SURVEY.md App. C
    for (mode, gi, ge) in ((3, 11, 1), (1, 11, 1), (4, 4.73, 0.34)):
        add("known_m%d" % mode, "PAWHEAE", "HEAGAWGHEE", mode, gi, ge, "fwd",
            ["opt", "cw", 10, 0.3, "1" * 12, "ucw", 10, 0.3], True)

    # B. small random pairs, every align_t, both directions, integer and non-integer gaps (+ empty / 1-residue sequences)
    rng = np.random.RandomState(20260)
    lens = [(0, 0), (0, 7), (5, 0), (1, 1), (1, 9), (8, 1), (2, 2)] + [(int(rng.randint(3, 34)), int(rng.randint(3, 34))) for _ in range(7)]
    for n, (ql, tl) in enumerate(lens):
        g = MT19937(7000 + n)
        q, t = residues(g, ql), residues(g, tl)
        for mode in range(5):
            for (gi, ge) in ((11, 1), (4.73, 0.34)):
                for d in ("fwd", "rev"):
                    add("small%02d_m%d_g%d_%s" % (n, mode, int(gi), d), q, t, mode, gi, ge, d, ["opt"], True)

    # C. near-optimal enumeration on mutated homologs
    for n in range(10):
        ln = int(rng.randint(12, 64))
        q, t = homolog_pair(8000 + n, ln, sub_rate=0.2, indel=3)
        T = len(t) + 2
        for mode in (1, 3, 4):
            gi, ge = ((11, 1), (4.73, 0.34))[n % 2]
            regs = int(rng.randint(1, 8))
            fl = "".join(str(int(x)) for x in orc.make_subopt_regions(T, regs))
            delta = float(rng.choice([0.01, 0.05, 0.1, 0.3]))
            nsub = int(rng.choice([3, 20, 40]))
            add("enum%02d_m%d" % (n, mode), q, t, mode, gi, ge, "fwd",
                ["opt", "cw", nsub, delta, fl, "ucw", nsub, delta], True,
                {"nsub": nsub, "delta": delta, "flags": fl})

    # D. 130 x 171 random pairs, hashes + optimal
    for n in range(3):
        q, t = random_pair(9000 + n, 130, 171)
        for mode in (1, 3, 4):
            add("mid%02d_m%d" % (n, mode), q, t, mode, 11, 1, "fwd", ["opt"], False)

    # E. config 1: seed 12345, two 300-aa sequences (query drawn first), modes 3/4/1, both gap settings
    q, t = random_pair(12345, 300)
    fl = "".join(str(int(x)) for x in orc.make_subopt_regions(302, 10))
    for mode in (3, 4, 1):
        for (gi, ge) in ((11, 1), (4.73, 0.34)):
            add("c1_m%d_g%d" % (mode, int(gi)), q, t, mode, gi, ge, "fwd", ["opt", "cw", 256, 0.05, fl], False,
                {"nsub": 256, "delta": 0.05, "flags": fl})
    # what the `aaa` driver enumerates without -opt: NOaliParams defaults (200, 0.01), every template flag set
    for mode, (gi, ge) in ((3, (11, 1)), (4, (4.73, 0.34))):
        add("aaa_m%d" % mode, q, t, mode, gi, ge, "fwd", ["opt", "cw", 200, 0.01, "1" * 302], False,
            {"nsub": 200, "delta": 0.01, "flags": "1" * 302}, sets_full=True)
    # a 300-aa homolog pair for long tracebacks + big enumerations (C4-shaped, small)
    q, t = homolog_pair(4242, 300)
    for mode in (3, 1):
        add("c4_m%d" % mode, q, t, mode, 11, 1, "fwd", ["opt", "cw", 256, 0.05, fl], False,
            {"nsub": 256, "delta": 0.05, "flags": fl})

    # F. sub-matrix builds (7-arg ctor) + Optimal_Subali
    subs = []
    for n in range(16):
        g = MT19937(9500 + n)
        ql, tl = int(rng.randint(6, 26)), int(rng.randint(6, 26))
        q, t = residues(g, ql), residues(g, tl)
        Q, T = ql + 2, tl + 2
        q1 = int(rng.randint(0, Q - 2)); q2 = int(rng.randint(q1 + 1, Q))
        t1 = int(rng.randint(0, T - 2)); t2 = int(rng.randint(t1 + 1, T))
        mode = (1, 3, 4)[n % 3]
        for d in ("fwd", "rev"):
            r = refrun.run_sub(q, t, mode, 11, 1, d, q1, t1, q2, t2)
            name = "sub%02d_%s" % (n, d)
            c = {"name": name, "q": q, "t": t, "mode": mode, "gi": 11, "ge": 1, "dir": d, "bounds": [q1, q2, t1, t2]}
            for k in ("H", "PQ", "PT"):
                arrays["%s/%s" % (name, k)] = r[k]
            if "subali" in r:
                c["subali"] = {"score": bits(r["subali"]["score"]), "pairs": r["subali"]["pairs"].reshape(-1).tolist()}
            if "throw" in r:
                c["throw"] = r["throw"]
            subs.append(c)

    with open(os.path.join(GOLD, "aa_cases.json"), "w") as f:
        json.dump({"generator": "oracle/gen_golden.py via oracle/_ref/ref_harness (real reference, g++ -O2, no -ffast-math)",
                   "cases": cases, "subs": subs}, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(GOLD, "aa_cases.npz"), **arrays)
    print("cases", len(cases), "subs", len(subs), "arrays", len(arrays))


def gen_profiles():
    """Profile path: real hmath.h + SimilarityMatrix + DPMatrix + Optimal driven by the plugin evaluator of
    oracle/ref_profile.cpp (Hmap2Eval itself needs the absent Troll library).  Inputs and outputs in one npz."""
    from aln_amd.synth import random_profile
    arrays = {}
    meta = []
    # (a 1 x 1 interior has zero variance: hmath.h:53 asserts and the reference aborts)
    shapes = [(1, 2), (3, 9), (17, 12), (40, 33), (64, 70)]
    for n, (ql, tl) in enumerate(shapes):
        qp, tp = random_profile(9700 + n, ql), random_profile(9800 + n, tl)
        for mode in range(5):
            for d in (1, 2):
                if d == 2 and mode not in (1, 3):
                    continue
                name = "prof%02d_m%d_d%d" % (n, mode, d)
                r = refrun.run_profile(qp, tp, mode, 0.5, 1.0, 0.12, 4.73, 0.34, d)
                for k in ("S", "H", "PQ", "PT", "TGI", "TGE", "PRIM"):
                    arrays[name + "/" + k] = r[k]
                m = {"name": name, "inputs": "in%02d" % n, "mode": mode, "dir": d, "alpha": 0.5, "beta": 1.0, "zero_shift": 0.12,
                     "gi": 4.73, "ge": 0.34}
                if "OPT" in r["sets"]:
                    a = r["sets"]["OPT"]["alis"][0]
                    m["opt"] = {"score": bits(a["score"]), "pairs": a["pairs"].reshape(-1).tolist()}
                meta.append(m)
        for side, p in (("q", qp), ("t", tp)):
            for k in ("aa", "sse", "conf"):
                arrays["in%02d/%s_%s" % (n, side, k)] = p[k]
    with open(os.path.join(GOLD, "profile_cases.json"), "w") as f:
        json.dump({"generator": "oracle/gen_golden.py via oracle/_ref/ref_profile (real hmath.h/DPMatrix/Optimal + plugin evaluator)",
                   "cases": meta}, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(GOLD, "profile_cases.npz"), **arrays)
    print("profile cases", len(meta))


def save_npz_stable(path, arrays):
    """np.savez_compressed stamps every member with the current time; this writes the same container (np.load reads it) with a
    fixed stamp and the members in sorted order, so that the file regenerates byte for byte."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)


def gen_profile_params():
    """The profile path off its default parameters: every set of tests/hmap2_cases.PARAMS on the 5 x 11 and the 19 x 14 inputs of
    profile_cases.npz (in01, in02: the same seeds; the inputs are not stored again), global and local, forward."""
    from aln_amd.synth import random_profile
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from hmap2_cases import PARAMS
    shapes = {1: (3, 9), 2: (17, 12)}
    arrays = {}
    meta = []
    for n, (ql, tl) in sorted(shapes.items()):
        qp, tp = random_profile(9700 + n, ql), random_profile(9800 + n, tl)
        for pname, pr in PARAMS.items():
            for mode in (1, 3):
                name = "par%02d_%s_m%d" % (n, pname, mode)
                r = refrun.run_profile(qp, tp, mode, pr["alpha"], pr["beta"], pr["zero_shift"], pr["gi"], pr["ge"], 1)
                for k in ("S", "H", "PQ", "PT", "TGI", "TGE"):
                    arrays[name + "/" + k] = r[k]
                a = r["sets"]["OPT"]["alis"][0]
                meta.append({"name": name, "inputs": "in%02d" % n, "params": pname, "mode": mode, "dir": 1, "alpha": pr["alpha"],
                             "beta": pr["beta"], "zero_shift": pr["zero_shift"], "gi": pr["gi"], "ge": pr["ge"],
                             "opt": {"score": bits(a["score"]), "pairs": a["pairs"].reshape(-1).tolist()}})
    with open(os.path.join(GOLD, "profile_param_cases.json"), "w") as f:
        json.dump({"generator": "oracle/gen_golden.py via oracle/_ref/ref_profile (real hmath.h/DPMatrix/Optimal + plugin evaluator)",
                   "inputs": "tests/golden/profile_cases.npz", "cases": meta}, f, separators=(",", ":"), sort_keys=True)
    save_npz_stable(os.path.join(GOLD, "profile_param_cases.npz"), arrays)
    print("profile parameter cases", len(meta))


def gen_enum_modes():
    """ConstrainedNearOptimal / UnconstrainedNearOptimal of the real reference in the two one-sided align types (0 and 2): the
    constant-gap small cases of tests/enum_mode_cases.py at 11/1 and 4.73/0.34, with that module's search parameters.  Writes
    tests/golden/enum_modes.json alone (aa_cases.* are not touched): plane digests, the Optimal set, and the CW and UCW sets
    with the first 6 pair lists in full."""
    if not refrun.available():
        raise SystemExit("oracle/_ref/ref_harness missing: run `make -C oracle` where the reference exists")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import enum_mode_cases as em
    cases = []
    for c, mode, fam in em.golden_runs():
        gi, ge = em.CONST[fam]
        cw, ucw = em.params(c, fam, "cw"), em.params(c, fam, "ucw")
        fl = "".join(str(int(x)) for x in em.flags(c, fam, "cw"))
        r = refrun.run_aa(c.q, c.t, mode, gi, ge, "fwd", ops=["dump", "opt", "cw", cw["nsub"], cw["delta"], fl, "ucw", ucw["nsub"], ucw["delta"]])
        assert "throw" not in r and set(r["sets"]) == {"OPT", "CW", "UCW"}, (c.name, mode, fam, r.get("throw"))
        cases.append({"name": em.golden_name(c, mode, fam), "case": c.name, "q": c.q, "t": c.t, "mode": mode, "gi": gi, "ge": ge, "dir": "fwd",
                      "flags": fl, "nsub": cw["nsub"], "delta": {"CW": cw["delta"], "UCW": ucw["delta"]},
                      "sha": {"H": sha(r["H"]), "PQ": sha(r["PQ"]), "PT": sha(r["PT"])},
                      "sets": {k: set_json(v, 6) for k, v in sorted(r["sets"].items())}})
    with open(os.path.join(GOLD, "enum_modes.json"), "w") as f:
        json.dump({"generator": "oracle/gen_golden.py enum_modes via oracle/_ref/ref_harness (real reference, g++ -O2, no -ffast-math)",
                   "cases": cases}, f, separators=(",", ":"), sort_keys=True)
    print("enum mode cases", len(cases))


def gen_enum_chain():
    """Two enumerations in a row on ONE AlignmentSet of the real reference (the harness's chain / chain0 ops): the chains of
    tests/enum_pool_cases.py.  The second call appends to what the first left, which is what aln_noa.n_existing > 1 promises.
    Writes tests/golden/enum_chain.json alone: the set after every step, the first 2 pair lists in full."""
    if not refrun.available():
        raise SystemExit("oracle/_ref/ref_harness missing: run `make -C oracle` where the reference exists")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import enum_pool_cases as ep
    cases = []
    for c in ep.chain_runs():
        ops = ["chain0" if c.empty else "chain", len(c.steps)]
        steps = []
        for kind, nsub, delta, regions in c.steps:
            fl = "".join(str(int(x)) for x in ep.flags(c.pair, regions))
            ops += [kind, nsub, delta] + ([fl] if kind == "cw" else [])
            steps.append({"kind": kind, "nsub": nsub, "delta": delta, "flags": fl})
        r = refrun.run_aa(c.pair.q, c.pair.t, c.mode, c.gap[0], c.gap[1], "fwd", ops=ops)
        want = {"CHAIN%d" % (k + 1) for k in range(len(c.steps))}
        assert "throw" not in r and set(r["sets"]) == want, (c.name, r.get("throw"))
        cases.append({"name": c.name, "q": c.pair.q, "t": c.pair.t, "mode": c.mode, "gi": c.gap[0], "ge": c.gap[1], "dir": "fwd",
                      "empty": c.empty, "steps": steps, "sets": {k: set_json(v, 2) for k, v in sorted(r["sets"].items())}})
    with open(os.path.join(GOLD, "enum_chain.json"), "w") as f:
        json.dump({"generator": "oracle/gen_golden.py enum_chain via oracle/_ref/ref_harness (real reference, g++ -O2, no -ffast-math)",
                   "cases": cases}, f, separators=(",", ":"), sort_keys=True)
    print("enum chain cases", len(cases))


if __name__ == "__main__":
    if sys.argv[1:] == ["profile_params"]:
        gen_profile_params()
    elif sys.argv[1:] == ["enum_modes"]:
        gen_enum_modes()
    elif sys.argv[1:] == ["enum_chain"]:
        gen_enum_chain()
    else:
        main()
        gen_profiles()
        gen_profile_params()
        gen_enum_modes()
        gen_enum_chain()
