"""CPU only.  (1) The oracle's ConstrainedNearOptimal / UnconstrainedNearOptimal in the two one-sided align types (0 frees query
end gaps only, 2 template end gaps only) against tests/golden/enum_modes.json, the sets of the real reference: planes, Optimal,
CW and UCW bit for bit (scores, uids, pair lists, identities, gapped strings, annotations).  KSCW and CRCW stay unpinned: their
headers do not build on LP64.  (2) The cases of enum_mode_cases.py bite: every search the GPU tests of
test_gpu_enumerate_modes.py run meets the builder's conditions and shows the teeth its case names — above all, the mirrored
end-gap rule gives another set."""
import numpy as np
import pytest

import enum_mode_cases as em
import goldens
import orc


def test_golden_file_holds_the_builder_cases():
    gold = goldens.enum_mode_cases()
    assert sorted(gold) == sorted(em.golden_name(*r) for r in em.golden_runs())
    assert len(gold) == 24
    for c, mode, fam in em.golden_runs():
        g = gold[em.golden_name(c, mode, fam)]
        assert (g["q"], g["t"], g["mode"]) == (c.q, c.t, mode) and mode in em.MODES_ONE_SIDED
        assert (np.float32(g["gi"]), np.float32(g["ge"])) == tuple(np.float32(x) for x in em.CONST[fam])
        assert g["flags"] == "".join(str(int(x)) for x in em.flags(c, fam, "cw"))
        for key, kind in (("CW", "cw"), ("UCW", "ucw")):
            pr = em.params(c, fam, kind)
            assert (g["nsub"], g["delta"][key]) == (pr["nsub"], pr["delta"])
            assert g["sets"][key]["n"] >= 2


@pytest.mark.parametrize("name", list(em._SMALL))
def test_oracle_equals_reference_in_one_sided_modes(name):
    gold = goldens.enum_mode_cases()
    n_sets = 0
    for c, mode, fam in em.golden_runs():
        if c.name != name:
            continue
        g = gold[em.golden_name(c, mode, fam)]
        S, D, PQ, PT, sc, pl = em.planes(c, mode, fam)
        goldens.check_matrices(g, D, PQ, PT)
        s = orc.AliSet()
        s.push(pl, sc)
        s.identity(c.q, c.t)
        tl, qls = s.strings(c.q, c.t)
        goldens.check_set(g, "OPT", [s.get(0)], tl, qls, [orc.annot(s.get(0)["score"], s.get(0)["identity"])])
        for key, kind in (("CW", "cw"), ("UCW", "ucw")):
            f = em.search(c, mode, fam, kind)
            assert f.status == 0
            s = orc.AliSet()
            for a in f.alis:
                s.push(a["pairs"], a["score"], a["uid"])
            tl, qls = s.strings(c.q, c.t)
            goldens.check_set(g, key, f.alis, tl, qls, [orc.annot(a["score"], a["identity"]) for a in f.alis])
            n_sets += 1
    assert n_sets == 8


@pytest.mark.parametrize("name", list(em._SMALL) + ["trip2", "trip2_resume"])
def test_cases_bite(name):
    """status 0, under 5 s, at least 2 alignments, and the teeth — for every (case, mode, gap family, kind) a GPU test runs"""
    runs = [r for r in em.constant_runs() + em.position_runs() + em.trip2_runs() if r[0].name == name]
    assert len(runs) == {"trip2": 1, "trip2_resume": 1}.get(name, 2 * (4 + 4 + 2) + 5 * 4 * (3 if name.endswith("_over8") else 1))
    slowest = 0.0
    for c, mode, fam, kind in runs:
        slowest = max(slowest, em.check(c, mode, fam, kind).seconds)
    if not name.startswith("trip2"):
        em.check_distinct(em.case(name))
    print("%s: %d searches, the slowest %.6f s" % (name, len(runs), slowest))


def test_mirrored_rule_is_a_real_swap():
    """the stand-in for "free deletions and free insertions swapped": 2 - mode exchanges the two one-sided align types, and
    with them the two flags of range_cases.free_ends / orc.deletion / orc.insertion"""
    import range_cases as rc
    for mode in em.MODES_ONE_SIDED:
        assert rc.free_ends(2 - mode) == rc.free_ends(mode)[::-1] and rc.free_ends(mode)[0] != rc.free_ends(mode)[1]
        g, m = orc.Gap(mode, 11, 1), orc.Gap(2 - mode, 11, 1)
        fdel, fins = rc.free_ends(mode)
        assert (orc.deletion(g, 9, 9, 1, 2, 0, 5) == 0) == fdel and (orc.deletion(m, 9, 9, 1, 2, 0, 5) == 0) == fins
        assert (orc.insertion(g, 9, 9, 3, 8, 1, 2) == 0) == fins and (orc.insertion(m, 9, 9, 3, 8, 1, 2) == 0) == fdel


def test_pruned_scan_precondition_of_the_constant_families():
    for c in em.small_cases() + [em.trip2_case(), em.trip2_resume_case()]:
        for fam in em.CONST:
            assert em.pruned_scan_precondition(c, fam)
        assert not em.pruned_scan_precondition(c, "tpos")
