"""-m gpu parity tests of the four near-optimal enumerators (cw, ucw, kscw, crcw) where the free-end-gap rule is ONE-SIDED
(align types 0 and 2), under the position-dependent gap models (the un-pruned candidate scans), and past the first
1024-candidate trip of the one-wave constant-gap scan.  Cases, parameters and the oracle's sets come from enum_mode_cases.py;
tests/test_enum_mode_reference.py proves on the CPU that every case bites (the mirrored end-gap rule gives another set) and
pins the oracle's cw / ucw sets to the real reference.  Every comparison is bit for bit: set size, order, float32 score bit
patterns, uids, pair lists and identities."""
import numpy as np
import pytest

import aln_amd
import enum_mode_cases as em
import goldens
import gpu_util
import orc

pytestmark = pytest.mark.gpu

WAVES = ((1, "one_wave"), (0, "waves_auto"), (3, "waves3"))
KIND_WAVES = [(k, w, "%s-%s" % (k, n)) for k in ("cw", "ucw", "kscw") for w, n in WAVES] + [("crcw", None, "crcw")]


@pytest.fixture(params=KIND_WAVES, ids=[x[2] for x in KIND_WAVES])
def kind(request):
    """the enumerator, run in its one-wave kernel, with the default number of waves and with 3 (crcw has one kernel)"""
    k, waves, _ = request.param
    if waves is None:
        yield k
    else:
        with gpu_util.ctx().hints(enum_waves=waves):
            yield k


@pytest.fixture(scope="module")
def resident():
    """(mode, family, case names) -> resident batch with its planes built, shared by the parameters of a test"""
    made = {}

    def get(mode, fam, cs):
        key = (mode, fam, tuple(c.name for c in cs))
        if key not in made:
            b = aln_amd.Batch(gpu_util.ctx(), [c.q for c in cs], [c.t for c in cs])
            kw = em.device_gap(cs, fam, mode)
            if fam in em.CONST or fam == "tpos":
                b.dp_submatrix(em.ALPHA, em.BLOSUM, mode, kw.pop("gi"), kw.pop("ge"), **kw)
            else:
                b.dp_simmatrix([em.planes(c, mode, fam)[0] for c in cs], mode, kw.pop("gi"), kw.pop("ge"), **kw)
            made[key] = b
        return made[key]

    yield get
    for b in made.values():
        b.close()


def _flag_rows(cs, fam, kind):
    rows = np.zeros((len(cs), max(em.dims(c)[1] for c in cs)), dtype=np.uint8)
    for p, c in enumerate(cs):
        rows[p, :em.dims(c)[1]] = em.flags(c, fam, kind)
    return rows


def _search_kw(c, fam, kind):
    pr = em.params(c, fam, kind)
    kw = dict(user_limit=pr["user_limit"])
    if kind in ("kscw", "crcw"):
        kw.update(k_limit=em.K_LIMIT)
    if kind == "crcw":
        kw.update(sort_limit=em.SORT_LIMIT, max_overlap=em.MAX_OVERLAP)
    return pr, kw


def _enumerate_one(b, p, c, fam, kind, want):
    pr, kw = _search_kw(c, fam, kind)
    assert pr["user_limit"] > 0
    return b.enumerate(p, kind, pr["nsub"], pr["delta"], em.flags(c, fam, kind), max_alignments=max(pr["nsub"], len(want)) + 2, **kw)


def _check_one(got, want, what):
    assert len(got) == len(want), what + (len(got), len(want))
    for k, (g, r) in enumerate(zip(got, want)):
        assert np.float32(g["score"]).view(np.uint32) == r["score"].view(np.uint32), what + (k, g["score"], r["score"])
        assert g["uid"] == r["uid"], what + (k, g["uid"], r["uid"])
        assert np.array_equal(g["pairs"], r["pairs"]), what + (k,)
        assert np.float32(g["identity"]).view(np.uint32) == r["identity"].view(np.uint32), what + (k,)


def _check_batch(b, mode, fam, cs, kind):
    """every pair through aln_batch_enumerate, the whole batch through aln_batch_enumerate_all with per-pair flag rows; each
    against the oracle and against the other -> the one-pair sets"""
    wants = [em.search(c, mode, fam, kind).alis for c in cs]
    ones = []
    for p, c in enumerate(cs):
        got = _enumerate_one(b, p, c, fam, kind, wants[p])
        _check_one(got, wants[p], (kind, mode, fam, c.name))
        ones.append(got)
    pr, kw = _search_kw(cs[0], fam, kind)
    assert all(_search_kw(c, fam, kind) == (pr, kw) for c in cs)
    n_out, scores, lengths, lists, status = b.enumerate_all(kind, pr["nsub"], pr["delta"], _flag_rows(cs, fam, kind), K=pr["nsub"] + 2,
                                                             node_cap=1 << 20, ali_cap=1 << 16, **kw)
    assert (status == 0).all(), (kind, mode, fam, status)
    for p, c in enumerate(cs):
        what = (kind, mode, fam, c.name, "batched")
        assert n_out[p] == len(wants[p]) == len(ones[p]), what + (n_out[p], len(wants[p]))
        for k, (r, o) in enumerate(zip(wants[p], ones[p])):
            assert scores[p, k].view(np.uint32) == r["score"].view(np.uint32), what + (k,)
            assert np.array_equal(lists[p, k, :lengths[p, k]], r["pairs"]), what + (k,)
            assert scores[p, k].view(np.uint32) == np.float32(o["score"]).view(np.uint32), what + (k,)
            assert np.array_equal(lists[p, k, :lengths[p, k]], o["pairs"]), what + (k,)
    return ones


def test_one_sided_modes_constant_gaps(kind, resident):
    """Align types 0 and 2 on the six flanked pairs under constant gaps 11/1, 4.73/0.34 (all kinds) and 0/0 (cw and kscw,
    user_limit 40: the edge of the pruned scans' gi >= 0 && ge >= 0 guard); cw and ucw also against the real reference.
    (crcw, t_tail140, align type 0, 4.73/0.34 is the case that showed the redundancy filter rejecting two sub-paths for their
    common end cell alone, crcw.h:440-455: 4 alignments instead of 5.)"""
    cs = em.small_cases()
    gold = goldens.enum_mode_cases()
    n_gold = 0
    for mode in em.MODES_ONE_SIDED:
        for fam in em.CONST:
            if kind not in em.kinds(fam):
                continue
            assert all(em.pruned_scan_precondition(c, fam) for c in cs)          # constant model, gi, ge >= 0, lengths <= 4096
            ones = _check_batch(resident(mode, fam, cs), mode, fam, cs, kind)
            if kind in ("cw", "ucw") and fam in em.GOLDEN_FAMILIES:
                for c, got in zip(cs, ones):
                    tl, qls, idn = gpu_util.strings_for(c.q, c.t, [g["pairs"] for g in got])
                    ann = [orc.annot(g["score"], g["identity"]) for g in got]
                    goldens.check_set(gold[em.golden_name(c, mode, fam)], kind.upper(), got, tl, qls, ann)
                    n_gold += 1
    assert n_gold == (24 if kind in ("cw", "ucw") else 0)


def test_one_sided_modes_position_gaps(kind, resident):
    """All five align types under ALN_GAP_AFFINE_TPOS_MIN (six pairs), ALN_GAP_DEL_TABLE_INS_TPOS and ALN_GAP_TABLES (the two
    *_over8 pairs): the un-pruned scans of all four kinds."""
    names = {"tpos": ("dp_exact_blocked", "dp_exact_tiled"), "gn2": ("dp_exact_tiled_kernel<gn2tab",), "tables": ("dp_exact_kernel",)}
    for mode in em.MODES_ALL:
        for fam in em.POSITION:
            cs = em.small_cases() if fam == "tpos" else em.over8_cases()
            assert not any(em.pruned_scan_precondition(c, fam) for c in cs)
            b = resident(mode, fam, cs)
            assert any(n in b.kernel_name() for n in names[fam]), (fam, b.kernel_name())
            _check_batch(b, mode, fam, cs, kind)


@pytest.mark.parametrize("waves", [1, 0], ids=["one_wave", "waves_auto"])
@pytest.mark.parametrize("name", ["trip2", "trip2_resume"])
def test_second_scan_trip(name, waves, resident):
    """trip2 (1042 x 902), align type 0, 11/1, cw: the accepted candidate of the final cell has scan index 1039 (asserted on the
    oracle by enum_mode_cases.check), beyond the 1024 candidates the one-wave constant-gap scan reads per trip; with the default
    hint the same candidate lies in a later chunk of the several-wave kernel's list.  trip2_resume: the same planes at delta
    0.03, where the final cell's scan accepts candidates on both sides of index 1024 and resumes from its cursor in between."""
    (c, mode, fam, kind), = [r for r in em.trip2_runs() if r[0].name == name]
    assert em.pruned_scan_precondition(c, fam)
    want = em.check(c, mode, fam, kind).alis
    b = resident(mode, fam, [em.trip2_case()])                                  # one resident batch for both searches
    with gpu_util.ctx().hints(enum_waves=waves):
        got = _enumerate_one(b, 0, c, fam, kind, want)
    _check_one(got, want, (kind, mode, fam, c.name, waves))
