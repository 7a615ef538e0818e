"""Cases and the float64 reference of syntax-aware segmentation: the
semi-Markov dynamic programme whose state is (frame, last category), with a
first-order chain over the categories of consecutive segments
(``abcd_span_table``, ``abcd_span_chain_viterbi``, ``segment_frames(transitions=
...)``).  ``span_cases`` is imported and left as it is.

The recurrence, in fp64 with every addition as written (fp32 inputs widened):

    G[0] = 0;  G[n] = G[n-1] + gap[n-1]           (gap None: -inf for n >= 1)
    W[0][k] = -inf
    U[n][k]  = max(G[n] + log_init[k], max_k' (W[n][k'] + log_trans[k'][k]))
    Vs[n][k] = max_{d_min <= d <= min(D,n)} (U[n-d][k] + T[n,d,k]) + seg_bonus
    W[n][k]  = max(W[n-1][k] + gap[n-1], Vs[n][k])
    path_score = max(G[N], max_k W[N][k])

NaN and -inf candidates are excluded.  Ties: the smallest d in Vs; the gap in W;
the initial term in U, then the lowest k'; at the end "no segment", then the
lowest k."""
import functools

import numpy as np

import span_cases as SP

NEG = SP.NEG

CHAIN_ND = ((1, 1), (2, 1), (33, 5), (33, 37), (70, 17))
CHAIN_K = (1, 2, 33, 65, 130)
CHAIN_KINDS = ("random", "tied", "holes", "gaps", "zeros", "nopath", "bonus")
TABLE_D = (1, 5, 17, 37)


def table_shapes():
    """(N, D) of the abcd_span_table cases: span_cases' shapes at D in TABLE_D (D = 37 > N = 33 among them)."""
    return [(n, d) for n, d in SP.abi_shapes() if d in TABLE_D]


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def chain_reference(table, d_min, log_trans, log_init, gap=None, seg_bonus=0.0):
    """The recurrence above in a float64 loop over n (the maxima over d and k'
    as elementwise numpy additions, the first maximum taken: the smallest d,
    the lowest k'): dict(W (N + 1 x K), path_score, onset, length, cat, score,
    link (lists in time order))."""
    T = np.asarray(table, dtype=np.float64)
    N, D, K = T.shape[0] - 1, T.shape[1], T.shape[2]
    lt, li = _f32(log_trans), _f32(log_init)
    g = None if gap is None else _f32(gap)
    bonus = np.float64(seg_bonus)
    G = np.zeros(N + 1)
    W = np.full((N + 1, K), NEG)
    U = np.full((N + 1, K), NEG)
    back_d = np.zeros((N + 1, K), dtype=np.int64)
    back_k = np.full((N + 1, K), -1, dtype=np.int64)
    U[0] = li
    cols = np.arange(K)
    with np.errstate(invalid="ignore"):
        for n in range(1, N + 1):
            G[n] = G[n - 1] + (g[n - 1] if g is not None else NEG)
            hi = min(D, n)
            best = np.full(K, NEG)
            bd = np.zeros(K, dtype=np.int64)
            if hi >= d_min:
                c = U[n - d_min:(n - hi - 1 if n > hi else None):-1] + T[n, d_min - 1:hi]     # (d, k)
                c = np.where(np.isnan(c), NEG, c)
                i = c.argmax(0)                       # the first maximum: the smallest d
                best, bd = c[i, cols], d_min + i
            seg = best + bonus
            gapc = W[n - 1] + g[n - 1] if g is not None else np.full(K, NEG)
            vg, vs = gapc > NEG, (seg > NEG) & (best > NEG)
            take_g = vg & (~vs | (gapc >= seg))
            W[n] = np.where(take_g, gapc, np.where(vs, seg, NEG))
            back_d[n] = np.where(take_g, 0, np.where(vs, bd, 0))
            if n == N:
                break
            c = W[n][:, None] + lt                    # (k', k)
            c = np.where(np.isnan(c), NEG, c)
            i = c.argmax(0)                           # the lowest k'
            best = c[i, cols]
            init = G[n] + li
            vi, vp = init > NEG, best > NEG
            take_i = vi & (~vp | (init >= best))
            U[n] = np.where(take_i, init, np.where(vp, best, NEG))
            back_k[n] = np.where(take_i, -1, np.where(vp, i, -1))
    best, kb = (G[N] if G[N] > NEG else NEG), -1
    for k in range(K):
        if N and W[N, k] > best:
            best, kb = W[N, k], k
    out = dict(W=W, path_score=float(best), onset=[], length=[], cat=[], score=[], link=[])
    n, k = N, kb
    while k >= 0 and n > 0:
        d = int(back_d[n, k])
        if d == 0:
            n -= 1
            continue
        out["onset"].append(n - d)
        out["length"].append(d)
        out["cat"].append(k)
        out["score"].append(float(T[n, d - 1, k]))
        n -= d
        p = int(back_k[n, k])
        out["link"].append(float(li[k] if p < 0 else lt[p, k]))
        k = p
    for key in ("onset", "length", "cat", "score", "link"):
        out[key].reverse()
    return out


def terms_of(ref_or_out, N, gap, seg_bonus):
    """(sum, sum of absolute values) of a path's own terms: score + link +
    bonus per segment and the gap of every uncovered frame."""
    covered = np.zeros(N, dtype=bool)
    terms = []
    for s, d, v, l in zip(ref_or_out["onset"], ref_or_out["length"], ref_or_out["score"], ref_or_out["link"]):
        covered[s:s + d] = True
        terms += [v, l, float(seg_bonus)]
    if not covered.all():
        terms += _f32(gap)[~covered].tolist()
    t = np.asarray(terms, dtype=np.float64)
    return float(t.sum()), float(np.abs(t).sum())


def context_free(table, lw):
    """(span_score, span_cat) N + 1 x D: the maximum over k of table + lw and
    the lowest k attaining it (-inf / -1 where nothing is left), what
    abcd_span_scores hands the context-free programme."""
    v = np.asarray(table, dtype=np.float64) + np.asarray(lw, dtype=np.float64)[None, None, :]
    v = np.where(np.isnan(v), NEG, v)
    score = v.max(-1)
    cat = np.where(score > NEG, v.argmax(-1), -1)
    return score, cat


def mask_impossible(T):
    """d > e holds -inf, as abcd_span_table writes it."""
    for e in range(min(T.shape[0], T.shape[1])):
        T[e, e:] = NEG
    return T


def random_table(g, N, D, K, scale=3.0):
    return mask_impossible(g.normal(0.0, scale, size=(N + 1, D, K)))


def log_softmax(v):
    v = np.asarray(v, dtype=np.float64)
    m = v.max()
    return v - (m + np.log(np.exp(v - m).sum()))


@functools.lru_cache(maxsize=None)
def chain_inputs(N, D, K, kind):
    """The inputs of one abcd_span_chain_viterbi case and the calls made on
    them: dict(table, trans, init, calls = [(d_min, gap, seg_bonus, tag)]).
    Shared, never modified.

    random  N(0, 3) table, drawn finite gap, dense chain
    tied    small integers everywhere (table, gap, chain, bonus): every sum is
            exact and every kind of tie occurs
    holes   the random table with NaN and -inf entries and whole rows of them
    gaps    no gap, a constant gap, the drawn gap, a gap with -inf entries
    zeros   the chain with structural zeros, NaN entries, a row of all zeros
            and a zero initial entry
    nopath  a chain of zeros only (one segment at most), with and without an
            initial distribution, with and without a gap
    bonus   nonzero seg_bonus"""
    g = np.random.default_rng(104729 * N + 1301 * D + 17 * K + CHAIN_KINDS.index(kind))
    if kind == "tied":
        T = mask_impossible(g.integers(-3, 2, size=(N + 1, D, K)).astype(np.float64))
        gap = g.integers(-2, 1, size=N).astype(np.float32)
        trans = g.integers(-2, 1, size=(K, K)).astype(np.float32)
        init = g.integers(-2, 1, size=K).astype(np.float32)
    else:
        T = random_table(g, N, D, K)
        gap = g.normal(-1.0, 1.0, size=N).astype(np.float32)
        trans = np.stack([log_softmax(g.normal(0.0, 2.0, size=K)) for _ in range(K)]).astype(np.float32)
        init = log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)
    if kind == "holes":
        T[g.random(T.shape) < 0.15] = np.nan
        T[g.random(T.shape) < 0.15] = NEG
        for r in g.integers(0, N + 1, size=max(N // 8, 1)):
            T[r] = np.nan if r % 2 else NEG
        mask_impossible(T)
    if kind == "zeros":
        trans[g.random(trans.shape) < 0.3] = NEG
        trans[g.random(trans.shape) < 0.05] = np.nan
        trans[K // 2] = NEG                          # a category nothing may follow
        init[K - 1] = NEG
    d_mins = sorted({1, min(3, D), D})
    calls = []
    for d_min in d_mins:
        if kind == "tied":
            calls += [(d_min, gp, b, f"dmin{d_min}{nm}b{b}") for nm, gp in (("null", None), ("drawn", gap))
                      for b in (0.0, -1.0, 1.0)]
        elif kind == "gaps":
            holed = gap.copy()
            holed[g.random(N) < 0.2] = NEG
            calls += [(d_min, gp, 0.0, f"dmin{d_min}{nm}") for nm, gp in
                      (("null", None), ("const", np.full(N, -2.0, dtype=np.float32)), ("drawn", gap), ("holed", holed))]
        elif kind == "bonus":
            calls += [(d_min, gp, b, f"dmin{d_min}{nm}b{b}") for nm, gp in (("null", None), ("drawn", gap))
                      for b in (-1.5, 2.25)]
        elif kind == "nopath":
            calls += [(d_min, None, 0.0, f"dmin{d_min}null"), (d_min, gap, 0.0, f"dmin{d_min}drawn")]
        else:
            calls += [(d_min, None, 0.0, f"dmin{d_min}null"), (d_min, gap, 0.0, f"dmin{d_min}drawn")]
    out = dict(table=T, trans=trans, init=init, calls=calls)
    if kind == "nopath":
        out["trans"] = np.full((K, K), NEG, dtype=np.float32)
        out["init_none"] = np.full(K, NEG, dtype=np.float32)
    return out


# ----------------------------------------------------------------------------
# the planted alternation
# ----------------------------------------------------------------------------
ALT_L, ALT_SEGMENTS, ALT_D = 4, 7, 6
ALT_STAY = 0.001


@functools.lru_cache(maxsize=None)
def planted_alternation():
    """Two categories with IDENTICAL emissions that alternate with probability
    1 - ALT_STAY: dict(table (N + 1 x D x 2), trans, init, lw, N, D).  Spans of
    ALT_L frames that end on a multiple of ALT_L score -1, every other span
    -40 per frame, so the cut is ALT_SEGMENTS segments of ALT_L frames under
    either programme; only the chain can tell the two categories apart."""
    N, D = ALT_L * ALT_SEGMENTS, ALT_D
    base = np.zeros((N + 1, D))
    for e in range(N + 1):
        for d in range(1, D + 1):
            base[e, d - 1] = -1.0 if (d == ALT_L and e % ALT_L == 0) else -40.0 * d
    T = mask_impossible(np.repeat(base[:, :, None], 2, axis=2))
    trans = np.log(np.array([[ALT_STAY, 1.0 - ALT_STAY], [1.0 - ALT_STAY, ALT_STAY]])).astype(np.float32)
    init = np.log(np.array([0.5, 0.5])).astype(np.float32)
    return dict(table=T, trans=trans, init=init, lw=np.log(np.array([0.5, 0.5])), N=N, D=D)


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as span_cases.dump)."""
    SP.PW.E.dump_observed("syntax_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/syntax_errors.json from a run of tests/test_gpu_syntax.py with
    ABCD_PARITY_DUMP=<dump_dir>."""
    import glob
    import json
    import os
    tab, e2e = [], []
    for path in sorted(glob.glob(os.path.join(dump_dir, "syntax_table_*.json"))):
        with open(path) as f:
            tab += json.load(f)
    for path in sorted(glob.glob(os.path.join(dump_dir, "syntax_e2e_*.json"))):
        with open(path) as f:
            e2e += json.load(f)
    doc = dict(what="figures observed by tests/test_gpu_syntax.py (ABCD_PARITY_DUMP) on one MI355X; units and bars: "
                    "tests/syntax_cases.py and tests/span_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(table=SP.BAR, best_and_argmax="equality with abcd_span_scores", chain_viterbi="equality",
                         path_vs_terms=1e-9, reduction_path_score=1e-9),
               worst=dict(table=max(r["table"] for r in tab),
                          reduction_path_score=max((r["reduction"] for r in e2e if "reduction" in r), default=None),
                          path_vs_terms=max((r["terms"] for r in e2e if "terms" in r), default=None)),
               table=tab, e2e=e2e)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/syntax_cases.py <dump directory> <out.json> <date> <parent commit>
    import sys
    print(assemble(*sys.argv[1:5])["worst"])
