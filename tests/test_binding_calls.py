"""What the search family's bindings (aln_amd, score_all_vs_all .. align_hits) hand to libalnhip.so and make of what comes back,
without a library or a GPU: aln_amd._LIB is replaced by a recorder that notes every call — the entry, every scalar, the fields
and pointed-to contents of every input struct and array, which optional pointers are NULL — fills the outputs from a counter
and returns a chosen status.  The records, the functions' results (or what they raised), their signatures and their docstrings
are compared with tests/golden/binding_calls.json.  `python tests/test_binding_calls.py` writes that file."""
import ctypes as C
import inspect
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_calls.json")
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "alignment-algos_amd"))

import aln_amd

ALPHABET = "ACDE"
TABLE = [[4, -1, -2, 0], [-1, 5, -3, 1], [-2, -3, 6, -1], [0, 1, -1, 3]]
QUERIES = ["", "ACDE", "DEACCADEA"]                       # lengths 0, 4, 9
TEMPLATES = ["A", "CDEAC", "EEDCADCA", "ACDEACDEACDE"]    # lengths 1 .. 12
K, Q_BEGIN, ROWS = 2, 1, 2
E_ARG, E_OVERFLOW = -5, -11

PUBLIC = ["score_all_vs_all", "search_topk", "profiles_from_sequences", "profile_planes", "score_profiles_vs_all",
          "search_topk_profiles", "shuffle_order", "shuffle_query", "hits_zscores", "hits_zscores_profiles", "hits_align",
          "hits_align_profiles", "hits_align_multi", "hits_align_multi_profiles", "masked_plane", "hits_align_multi_detour",
          "hits_align_multi_profiles_detour", "hits_column_counts", "hits_column_counts_profiles", "pssm_from_counts",
          "hits_align_routes", "align_hits"]


def _struct(a):
    """the struct behind a byref() argument or a pointer, None for NULL"""
    if a is None:
        return None
    return a._obj if hasattr(a, "_obj") else a.contents


def _values(a, ctype, n):
    if a is None:
        return None
    p = C.cast(a, C.POINTER(ctype))
    return [p[i] for i in range(n)]


def _is_null(p):
    return p is None or not bool(p)


class Recorder:
    """Stands in for the loaded library: every aln_* entry of the family is a method that records and fills."""

    def __init__(self, rc=0, carried=False):
        self.rc, self.carried, self.calls, self.counter = rc, carried, [], 0

    def tick(self):
        self.counter += 1
        return self.counter

    def aln_error_string(self, rc):
        return ("status %d" % rc).encode()

    def aln_last_error(self, h):
        return b"last error"

    # ---- inputs ----
    def seqs(self, a):
        s = _struct(a)
        if s is None:
            return None
        off = [s.offsets[i] for i in range(s.n_seqs + 1)]
        return {"n_seqs": s.n_seqs, "offsets": off, "residues": C.string_at(s.residues, off[-1]).decode()}

    def sub(self, a):
        s = _struct(a)
        return {"n": s.n, "alphabet": s.alphabet.decode(), "table": [s.table[i] for i in range(s.n * s.n)]}

    def gap(self, a):
        g = _struct(a)
        d = {k: getattr(g, k) for k in ("model", "align_type", "gap_init", "gap_extn", "dp_local")}
        d["null"] = [k for k in ("t_gap_init", "t_gap_extn", "t_gap_cn", "del_table", "del_table_off", "ins_tables", "ins_table_off")
                     if _is_null(getattr(g, k))]
        return d

    def profiles(self, a):
        p = _struct(a)
        off = [p.offsets[i] for i in range(p.n_seqs + 1)]
        return {"n_seqs": p.n_seqs, "offsets": off, "n": p.n, "alphabet": p.alphabet.decode(),
                "rows": [p.rows[i] for i in range(off[-1] * p.n)]}

    def lead(self, rec, it, kind):
        """the arguments up to the gap; -> (number of templates, offsets of the query side, letters of the alphabet)"""
        rec["ctx"] = next(it).value
        if kind == "residue":
            rec["queries"] = self.seqs(next(it))
            qoff = rec["queries"]["offsets"]
        else:
            rec["profiles"] = self.profiles(next(it))
            qoff = rec["profiles"]["offsets"]
            if kind == "profile_consensus":
                rec["consensus"] = self.seqs(next(it))
        rec["templates"] = self.seqs(next(it))
        if kind == "residue":
            rec["sub"] = self.sub(next(it))
        rec["gap"] = self.gap(next(it))
        return rec["templates"]["n_seqs"], qoff, rec["sub"]["n"] if kind == "residue" else rec["profiles"]["n"]

    def scalars(self, rec, it, *names):
        for n in names:
            rec[n] = next(it)
        return [rec[n] for n in names]

    def hit_list(self, rec, it, rows, k):
        h = C.cast(next(it), C.POINTER(aln_amd.AlnHit))
        rec["hits"] = [[h[i].t, h[i].score, h[i].q_end, h[i].t_end] for i in range(rows * k)]
        rec["n_hits"] = _values(next(it), C.c_int32, rows)

    # ---- outputs ----
    def fill(self, rec, name, a, ctype, n, mod=97):
        rec[name + "_null"] = a is None
        if a is not None:
            p = C.cast(a, C.POINTER(ctype))
            for i in range(n):
                p[i] = self.tick() % mod

    def fill_records(self, a, n, pair_stride):
        p = C.cast(a, C.POINTER(aln_amd.AlnHitAlignment))
        for i in range(n):
            p[i].n_pairs = self.tick() % (pair_stride + 3)          # some beyond the stride: the lists are clipped
            p[i].status = self.rc if (self.carried and i == 1) else 0
            p[i].score = 0.5 * self.tick()
            p[i].identity = 0.125 * (self.tick() % 9)

    def fill_lines(self, rec, it, n):
        """pairs, pair_stride, tlines, qlines, line_stride, lengths"""
        pairs, pair_stride, tl, ql, line_stride, lengths = [next(it) for _ in range(6)]
        rec["pair_stride"], rec["line_stride"] = pair_stride, line_stride
        self.fill(rec, "pairs", pairs, C.c_int32, n * pair_stride * 2, 1000)
        rec["tlines_null"], rec["qlines_null"] = tl is None, ql is None
        self.fill(rec, "lengths", lengths, C.c_int32, n, max(line_stride, 1))
        for buf in (tl, ql):
            if buf is not None:
                p = C.cast(buf, C.POINTER(C.c_char))
                for i in range(n * line_stride):
                    p[i] = bytes([65 + self.tick() % 26])

    def done(self, rec, it):
        assert next(it, None) is None, "more arguments than the entry takes"
        self.calls.append(rec)
        return self.rc

    # ---- the entries ----
    def _score(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        n_t, _, _ = self.lead(rec, it, kind)
        qb, qe = self.scalars(rec, it, "q_begin", "q_end")
        p = C.cast(next(it), C.POINTER(C.c_float))
        for i in range((qe - qb) * n_t):
            p[i] = 0.25 * self.tick()
        return self.done(rec, it)

    def _search(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        self.lead(rec, it, kind)
        qb, qe, k, _ = self.scalars(rec, it, "q_begin", "q_end", "K", "min_score")
        h = C.cast(next(it), C.POINTER(aln_amd.AlnHit))
        for i in range((qe - qb) * k):
            h[i].t, h[i].score, h[i].q_end, h[i].t_end = self.tick() % 4, 0.5 * self.tick(), self.tick() % 7, self.tick() % 11
        self.fill(rec, "n_hits_out", next(it), C.c_int32, qe - qb, k + 1)
        return self.done(rec, it)

    def _zscores(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        self.lead(rec, it, kind)
        qb, qe, k = self.scalars(rec, it, "q_begin", "q_end", "K")
        self.hit_list(rec, it, qe - qb, k)
        self.scalars(rec, it, "n_shuffles", "seed")
        s = C.cast(next(it), C.POINTER(aln_amd.AlnHitStats))
        for i in range((qe - qb) * k):
            s[i].sum, s[i].sumsq, s[i].n, s[i].z = self.tick(), self.tick() * 1000, self.tick() % 50, 0.25 * self.tick()
        return self.done(rec, it)

    def _align(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        self.lead(rec, it, kind)
        qb, qe, k = self.scalars(rec, it, "q_begin", "q_end", "K")
        self.hit_list(rec, it, qe - qb, k)
        out = next(it)
        rest = list(it)
        self.fill_records(out, (qe - qb) * k, rest[1])
        it = iter(rest)
        self.fill_lines(rec, it, (qe - qb) * k)
        return self.done(rec, it)

    def _multi(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        self.lead(rec, it, kind)
        qb, qe, k = self.scalars(rec, it, "q_begin", "q_end", "K")
        self.hit_list(rec, it, qe - qb, k)
        n, _ = self.scalars(rec, it, "max_alignments", "min_score")
        self.fill(rec, "n_found", next(it), C.c_int32, (qe - qb) * k, max(n, 1) + 1)
        out = next(it)
        rest = list(it)
        self.fill_records(out, (qe - qb) * k * max(n, 1), rest[1])
        it = iter(rest)
        self.fill_lines(rec, it, (qe - qb) * k * max(n, 1))
        return self.done(rec, it)

    def _counts(self, kind, name, args):
        rec, it = {"entry": name}, iter(args)
        _, qoff, n_alpha = self.lead(rec, it, kind)
        qb, qe, k = self.scalars(rec, it, "q_begin", "q_end", "K")
        self.hit_list(rec, it, qe - qb, k)
        rec["weights"] = _values(next(it), C.c_int32, (qe - qb) * k)
        self.fill_records(next(it), (qe - qb) * k, 5)
        n_rows = qoff[qe] - qoff[qb]
        self.fill(rec, "counts", next(it), C.c_int32, n_rows * n_alpha)
        self.fill(rec, "covered", next(it), C.c_int32, n_rows)
        return self.done(rec, it)

    def aln_hits_align_last_routes(self, h, out):
        rec = {"entry": "aln_hits_align_last_routes", "ctx": h.value}
        p = C.cast(out, C.POINTER(C.c_int64))
        p[0], p[1] = self.tick(), self.tick()
        self.calls.append(rec)
        return self.rc

    def __getattr__(self, name):
        table = {"aln_score_all_vs_all": (self._score, "residue"), "aln_score_profiles_vs_all": (self._score, "profile"),
                 "aln_search_topk": (self._search, "residue"), "aln_search_topk_profiles": (self._search, "profile"),
                 "aln_hits_zscores": (self._zscores, "residue"), "aln_hits_zscores_profiles": (self._zscores, "profile"),
                 "aln_hits_align": (self._align, "residue"), "aln_hits_align_profiles": (self._align, "profile_consensus"),
                 "aln_hits_align_multi": (self._multi, "residue"), "aln_hits_align_multi_profiles": (self._multi, "profile_consensus"),
                 "aln_hits_column_counts": (self._counts, "residue"),
                 "aln_hits_column_counts_profiles": (self._counts, "profile_consensus")}
        if name not in table:
            raise AttributeError(name)
        f, kind = table[name]
        return lambda *args: f(kind, name, args)


class FakeContext:
    h = C.c_void_p(0x1234)


def _plain(x):
    """a result as JSON can hold it"""
    if x is None or isinstance(x, (bool, int, str)):
        return x
    if isinstance(x, float):
        return x
    if isinstance(x, np.ndarray):
        return {"dtype": str(x.dtype) if x.dtype.names is None else list(x.dtype.names), "shape": list(x.shape),
                "values": _plain(x.tolist())}
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    raise TypeError(type(x))


def _hits():
    hits = np.zeros((ROWS, K), dtype=aln_amd.HIT_DTYPE)
    hits["t"] = [[3, 1], [2, -1]]
    hits["score"] = [[17.0, 9.0], [21.0, 0.0]]
    hits["q_end"] = [[4, 2], [9, -1]]
    hits["t_end"] = [[12, 3], [8, -1]]
    return hits, [2, 1]                                      # n_hits as a plain list: the binding makes it int32


def _cases():
    """name -> (function, args, kwargs, recorder arguments)"""
    A = aln_amd
    ctx = FakeContext()
    hits, n_hits = _hits()
    prof = A.profiles_from_sequences(QUERIES, ALPHABET, TABLE)
    cons = ["", "CCCC", "DDDDDDDDD"]
    tpool = A.SeqPool(TEMPLATES)
    res = (ctx, QUERIES, TEMPLATES)
    sub = (ALPHABET, TABLE, 11, 1)
    weights = [[3, 0], [65535, 1]]
    cases = {
        "score_all_vs_all": (A.score_all_vs_all, res + sub, dict(q_begin=Q_BEGIN), {}),
        "score_all_vs_all_range_pools": (A.score_all_vs_all, (ctx, A.SeqPool(QUERIES), tpool) + sub,
                                         dict(q_begin=Q_BEGIN, q_end=2, align_type=A.GLOBAL), {}),
        "score_all_vs_all_error": (A.score_all_vs_all, res + sub, dict(q_begin=Q_BEGIN), dict(rc=E_ARG)),
        "search_topk": (A.search_topk, res + sub + (K,), dict(q_begin=Q_BEGIN), {}),
        "search_topk_min_score": (A.search_topk, res + sub + (K,), dict(min_score=7.5, q_begin=Q_BEGIN, q_end=3, align_type=A.SEMI_LOCAL), {}),
        "search_topk_error": (A.search_topk, res + sub + (K,), dict(q_begin=Q_BEGIN), dict(rc=E_ARG)),
        "score_profiles_vs_all": (A.score_profiles_vs_all, (ctx, prof, TEMPLATES, 11, 1), dict(q_begin=Q_BEGIN), {}),
        "score_profiles_vs_all_range": (A.score_profiles_vs_all, (ctx, prof, tpool, 10.5, 0.5),
                                        dict(q_begin=Q_BEGIN, q_end=2, align_type=A.LOCAL_GLOBAL), {}),
        "search_topk_profiles": (A.search_topk_profiles, (ctx, prof, TEMPLATES, 11, 1, K), dict(q_begin=Q_BEGIN), {}),
        "search_topk_profiles_error": (A.search_topk_profiles, (ctx, prof, TEMPLATES, 11, 1, K),
                                       dict(min_score=3, q_begin=Q_BEGIN, q_end=3), dict(rc=E_ARG)),
        "hits_zscores": (A.hits_zscores, res + (hits, n_hits) + sub + (5,), dict(seed=(1 << 32) + 77, q_begin=Q_BEGIN), {}),
        "hits_zscores_error": (A.hits_zscores, res + (hits, n_hits) + sub + (5,), dict(q_begin=Q_BEGIN, align_type=A.GLOBAL), dict(rc=E_ARG)),
        "hits_zscores_profiles": (A.hits_zscores_profiles, (ctx, prof, TEMPLATES, hits, n_hits, 11, 1, 5),
                                  dict(seed=-1, q_begin=Q_BEGIN), {}),
        "hits_column_counts": (A.hits_column_counts, res + (hits, n_hits) + sub, dict(q_begin=Q_BEGIN), {}),
        "hits_column_counts_weights": (A.hits_column_counts, res + (hits, n_hits) + sub,
                                       dict(weights=weights, q_begin=Q_BEGIN, align_type=A.GLOBAL, want_covered=False),
                                       dict(rc=E_OVERFLOW, carried=True)),
        "hits_column_counts_error": (A.hits_column_counts, res + (hits, n_hits) + sub, dict(q_begin=Q_BEGIN), dict(rc=E_ARG)),
        "hits_column_counts_profiles": (A.hits_column_counts_profiles, (ctx, prof, TEMPLATES, hits, n_hits, 11, 1),
                                        dict(consensus=cons, weights=weights, q_begin=Q_BEGIN), {}),
        "hits_column_counts_profiles_plain": (A.hits_column_counts_profiles, (ctx, prof, tpool, hits, n_hits, 11, 1),
                                              dict(q_begin=Q_BEGIN, want_covered=False), dict(rc=E_ARG)),
        "hits_align_routes": (A.hits_align_routes, (ctx,), {}, {}),
        "align_hits_no_hit": (A.align_hits, res + (hits, [0, 0]) + sub, dict(q_begin=Q_BEGIN), {}),
        "shuffle_order": (lambda: [A.shuffle_order(s, q, k, n) for s, q, k, n in ((0, 0, 0, 0), (1, 2, 3, 1), (77, 1, 4, 9), (2 ** 32 - 1, 5, 0, 17))], (), {}, {}),
        "shuffle_query": (lambda: [A.shuffle_query(s, q, k, r) for s, q, k, r in ((0, 0, 0, ""), (1, 2, 3, "A"), (77, 1, 4, "DEACCADEA"), (2 ** 32 - 1, 5, 0, "ACDEACDEACDEACDEA"))], (), {}, {}),
        "profile_planes": (A.profile_planes, (prof.profiles[1], "CDEAC", ALPHABET), {}, {}),
        "masked_plane": (A.masked_plane, ("ACDE", "CDEAC", ALPHABET, TABLE, [(1, 2), (3, 3)], -18.0), {}, {}),
        "pssm_from_counts": (A.pssm_from_counts, ([[3, 0, 1, 0], [0, 0, 0, 0]], [0.4, 0.3, 0.2, 0.1], [[1, 2, 3, 4], [5, 6, 7, 8]]), {}, {}),
    }
    # the four alignment entries: lists and lines on and off, default and explicit strides, the three statuses
    align = {"hits_align": (A.hits_align, res + (hits, n_hits) + sub, {}),
             "hits_align_profiles": (A.hits_align_profiles, (ctx, prof, TEMPLATES, hits, n_hits, 11, 1), dict(consensus=cons)),
             "hits_align_multi": (A.hits_align_multi, res + (hits, n_hits) + sub + (3,), dict(min_score=5.0)),
             "hits_align_multi_profiles": (A.hits_align_multi_profiles, (ctx, prof, TEMPLATES, hits, n_hits, 11, 1, 3), dict(consensus=A.SeqPool(cons)))}
    for name, (f, args, kw) in align.items():
        base = dict(kw, q_begin=Q_BEGIN)
        plain = {k: v for k, v in base.items() if k != "consensus"}
        cases[name] = (f, args, base, {})
        cases[name + "_strides"] = (f, args, dict(base, pair_stride=4, line_stride=9, align_type=A.SEMI_LOCAL), dict(rc=E_OVERFLOW, carried=True))
        cases[name + "_records_only"] = (f, args, dict(plain, want_pairs=False, want_lines=False), {})
        cases[name + "_lines_only"] = (f, args, dict(plain, want_pairs=False, line_stride=7), {})
        cases[name + "_pairs_only"] = (f, args, dict(base, want_lines=False, pair_stride=3), dict(rc=E_OVERFLOW, carried=True))
        cases[name + "_error"] = (f, args, base, dict(rc=E_ARG))
    cases["hits_align_multi_none"] = (A.hits_align_multi, res + (hits, n_hits) + sub + (0,), dict(q_begin=Q_BEGIN), {})
    return cases


def _run(name, monkeypatch_setattr):
    f, args, kw, rkw = _cases()[name]
    rec = Recorder(**rkw)
    monkeypatch_setattr(aln_amd, "_LIB", rec)
    try:
        result = {"returned": _plain(f(*args, **kw))}
    except aln_amd.AlnError as e:
        result = {"raised": type(e).__name__, "code": e.code, "text": str(e)}
    return {"calls": rec.calls, "result": result}


def _normal(x):
    return json.loads(json.dumps(x))


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def pytest_generate_tests(metafunc):
    if "case" in metafunc.fixturenames:
        metafunc.parametrize("case", sorted(_cases()))
    if "public" in metafunc.fixturenames:
        metafunc.parametrize("public", PUBLIC)


def test_call_matches_the_record(case, monkeypatch):
    got = _normal(_run(case, monkeypatch.setattr))
    want = _golden()["cases"][case]
    assert got["calls"] == want["calls"]
    assert got["result"] == want["result"]


def test_every_recorded_case_is_run():
    assert sorted(_golden()["cases"]) == sorted(_cases())


def test_signature_and_docstring(public):
    f = getattr(aln_amd, public)
    want = _golden()["public"][public]
    assert str(inspect.signature(f)) == want["signature"]
    assert f.__doc__ == want["doc"]


def test_submatrix_and_gap_outlive_their_makers(monkeypatch):
    """The table and alphabet bytes a call's aln_submatrix points to are read by the recorder after a garbage collection."""
    import gc
    seen = {}

    class Collecting(Recorder):
        def sub(self, a):
            gc.collect()
            junk = [np.full(16, -7.0, dtype=np.float32) for _ in range(64)]      # reuse what a collected table would have freed
            seen["sub"] = Recorder.sub(self, a)
            del junk
            return seen["sub"]

    monkeypatch.setattr(aln_amd, "_LIB", Collecting())
    aln_amd.hits_align(FakeContext(), QUERIES, TEMPLATES, *_hits(), ALPHABET, [[float(v) for v in row] for row in TABLE], 11, 1, q_begin=Q_BEGIN)
    assert seen["sub"] == {"n": 4, "alphabet": ALPHABET, "table": [float(v) for row in TABLE for v in row]}


if __name__ == "__main__":
    def setattr_(obj, name, value):
        setattr(obj, name, value)
    doc = {"cases": {name: _run(name, setattr_) for name in sorted(_cases())},
           "public": {p: {"signature": str(inspect.signature(getattr(aln_amd, p))), "doc": getattr(aln_amd, p).__doc__} for p in PUBLIC}}
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True, separators=(",", ":"))
        fh.write("\n")
    print("%s: %d cases, %d bytes" % (GOLDEN, len(doc["cases"]), os.path.getsize(GOLDEN)))
