"""Cases, references and bars of the segmentation posteriors under the chain:
the semi-Markov forward-backward over (frame, last category)
(``abcd_span_chain_posterior``, ``ops.span_chain_posterior``,
``segmentation.segment_chain_posteriors`` / ``refit_transitions_em``,
``segment.py --chain_posteriors``).  ``syntax_cases`` supplies
the inputs (``chain_inputs``) and ``spanpost_cases`` the context-free reference
the reduction is checked against; both are imported and left as they are.

The recursions, in ``np.longdouble``.  T, gap, bonus, lt, li are the inputs
(fp32 ones widened) times ``scale``; a candidate that is NaN or -inf is
excluded; LAE is logaddexp, LSE the log-sum-exp, -inf over none:

    G[0] = 0;  G[n] = G[n-1] + gap[n-1]                  (gap None: -inf for n >= 1)
    aW[0][k] = aV[0][k] = -inf
    aU[n][k] = LAE(G[n] + li[k], LSE_k' (aW[n][k'] + lt[k'][k]))        n < N;  aU[N][k] = -inf
    aV[n][k] = bonus + LSE_{d_min<=d<=min(D,n)} (aU[n-d][k] + T[n,d,k])
    aW[n][k] = LAE(aW[n-1][k] + gap[n-1], aV[n][k])
    log_z    = LAE(G[N], LSE_k aW[N][k])
    bW[N][k] = 0, bG[N] = 0, bU[N][k] = -inf;  n = N-1 .. 0:
    bU[n][k] = LSE_{d_min<=d<=min(D,N-n)} (T[n+d,d,k] + bonus + bW[n+d][k])
    bW[n][k] = LAE(gap[n] + bW[n+1][k], LSE_k'' (lt[k][k''] + bU[n][k'']))
    bG[n]    = LAE(gap[n] + bG[n+1], LSE_k (li[k] + bU[n][k]))

and the posteriors and counts of DESIGN.md s3.14 from them.

Bars (derived, not tuned).  The lattice within ``lattice_bar``: 8 N (D + K + 2)
2^-53 (M + 1) absolute, M the largest finite |value| of the reference lattice:
s3.12's bar (a rounding per combine and a few ulp of libm, errors passed from
step to step with weight <= 1) with D + K candidates per step instead of D;
doubled when longdouble is not extended precision.  Posteriors within 5 lattice
bars absolute (exp of a sum of three lattice values minus log_z, each value <=
1).  A count entry within 5 lattice bars times (1 + its reference value): a sum
of terms whose relative error is the lattice error."""
import functools

import numpy as np

import spanpost_cases as PC
import syntax_cases as SX

NEG = -np.inf
LD = PC.LD
LD_OK = PC.LD_OK
RT = LD if LD_OK else np.float64

CHAIN_ND = SX.CHAIN_ND
CHAIN_K = SX.CHAIN_K
CHAIN_KINDS = SX.CHAIN_KINDS
WIDTH_K = (256, 257)           # across the launch-width threshold, at (33, 5)
SCALE = 0.25


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(RT)


def _clean(c):
    """NaN -> -inf"""
    return np.where(c > NEG, c, RT(NEG))


def _lse(c, axis=0):
    """LSE over ``axis`` of the candidates above -inf; -inf over none."""
    c = _clean(c)
    m = c.max(axis=axis)
    ms = np.where(m > NEG, m, RT(0))
    z = np.exp(c - np.expand_dims(ms, axis)).sum(axis=axis)
    with np.errstate(divide="ignore"):
        return np.where(m > NEG, ms + np.log(z), RT(NEG))


def _lae(a, b):
    return _lse(np.stack([np.asarray(a, dtype=RT), np.asarray(b, dtype=RT)]), 0)


def chain_posterior_reference(table, d_min, log_trans, log_init, gap=None, seg_bonus=0.0, scale=1.0,
                              want_table=True):
    """The recursions above, each step's candidates as one numpy array; the
    sums over k' go through E = exp(lt) once (LSE_k' (a[k'] + lt[k'][k]) = m +
    log(exp(a - m) @ E), exact to a few longdouble ulp: the terms are positive
    and longdouble's exponent range leaves no underflow), which keeps exp out
    of the K x K loops.  dict of float64 arrays log_z, lattice (5 x (N + 1) x K: aU, aV, aW, bU, bW),
    lattice_g (2 x (N + 1): G, bG), post_k (2 x (N + 1) x K: onset, end),
    gap_post (N + 1), trans_counts (K x K), init_counts (K), span_post ((N +
    1) x D, with want_table) and no_segment."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = RT(scale)
        T = np.asarray(table, dtype=np.float64).astype(RT) * s
        N, D, K = T.shape[0] - 1, T.shape[1], T.shape[2]
        lt, li = _f32(log_trans) * s, _f32(log_init) * s
        g = None if gap is None else _f32(gap) * s
        bonus, neg = RT(seg_bonus) * s, RT(NEG)
        E = np.exp(_clean(lt))                                                                   # 0 at structural zeros

        def shifted(v):
            """(exp(v - max v), max v) over the entries above -inf; (None, -inf) over none"""
            v = _clean(v)
            m = v.max()
            return (np.exp(v - m), m) if m > NEG else (None, neg)

        def through(v, into):
            """LSE_k' (v[k'] + lt[k'][k]) (into) or LSE_k'' (lt[k][k''] + v[k'']) (out of the row)"""
            w, m = shifted(v)
            if w is None:
                return np.full(K, neg)
            z = w @ E if into else E @ w
            return np.where(z > 0, m + np.log(np.where(z > 0, z, 1)), neg)
        G = np.full(N + 1, neg)
        G[0] = 0
        aU, aV, aW = (np.full((N + 1, K), neg) for _ in range(3))
        bU, bW = np.full((N + 1, K), neg), np.full((N + 1, K), neg)
        bG = np.full(N + 1, neg)
        if N > 0:
            aU[0] = _lae(G[0] + li, through(aW[0], True))
        for n in range(1, N + 1):
            gv = g[n - 1] if g is not None else neg
            G[n] = G[n - 1] + gv
            hi = min(D, n)
            if hi >= d_min:
                c = aU[n - d_min:(n - hi - 1 if n > hi else None):-1] + T[n, d_min - 1:hi]      # (d, k)
                aV[n] = _clean(bonus + _lse(c, 0))
            aW[n] = _lae(aW[n - 1] + gv, aV[n])
            if n < N:
                aU[n] = _lae(G[n] + li, through(aW[n], True))
        lz = _lae(G[N], _lse(aW[N], 0)) if N > 0 else RT(0)
        bW[N], bG[N] = 0, 0
        ix = np.arange(D)
        for n in range(N - 1, -1, -1):
            gv = g[n] if g is not None else neg
            hi = min(D, N - n)
            if hi >= d_min:
                d = ix[d_min - 1:hi]                                                             # d - 1
                bU[n] = _lse(T[n + d + 1, d] + bonus + bW[n + d + 1], 0)
            bW[n] = _lae(gv + bW[n + 1], through(bU[n], False))
            bG[n] = _lae(gv + bG[n + 1], _lse(li + bU[n], 0))
        reach = bool(lz > NEG)
        post_k = np.zeros((2, N + 1, K), dtype=RT)
        gap_post = np.zeros(N + 1, dtype=RT)
        tc, ic = np.zeros((K, K), dtype=RT), np.zeros(K, dtype=RT)
        span = np.zeros((N + 1, D), dtype=RT)
        no_seg = RT(0)
        if reach and N > 0:
            def ex(c):
                return np.where(c > NEG, np.exp(np.where(c > NEG, c, 0)), 0)
            post_k[0] = ex(aU + bU - lz)
            post_k[1] = ex(aV + bW - lz)
            if g is not None:
                inner = _lae(G[:N] + bG[1:], _lse(aW[:N] + bW[1:], 1))
                gap_post[:N] = ex(inner + g - lz)
            for n in range(N):
                ic += ex(G[n] + li + bU[n] - lz)
                (w, ma), (u, mb) = shifted(aW[n]), shifted(bU[n])
                if w is not None and u is not None:
                    tc += (w[:, None] * E * u[None, :]) * np.exp(ma + mb - lz)
            if want_table:
                for e in range(1, N + 1):
                    hi = min(D, e)
                    if hi >= d_min:
                        c = aU[e - d_min:(e - hi - 1 if e > hi else None):-1] + T[e, d_min - 1:hi] + bonus + bW[e]
                        span[e, d_min - 1:hi] = ex(c - lz).sum(1)
            no_seg = ex(G[N] - lz)
        f = np.float64
        return dict(log_z=float(lz), lattice=np.stack([aU, aV, aW, bU, bW]).astype(f),
                    lattice_g=np.stack([G, bG]).astype(f), post_k=post_k.astype(f), gap_post=gap_post.astype(f),
                    trans_counts=tc.astype(f), init_counts=ic.astype(f), span_post=span.astype(f),
                    no_segment=float(no_seg))


def brute_force(table, d_min, log_trans, log_init, gap=None, seg_bonus=0.0, scale=1.0):
    """Every labelled cover of N <= 9 frames enumerated in np.longdouble: dict
    of log_z, post_k, gap_post, trans_counts, init_counts, span_post,
    no_segment from the covers' weights."""
    T = np.asarray(table, dtype=np.float64)
    N, D, K = T.shape[0] - 1, T.shape[1], T.shape[2]
    assert N <= 9
    s = LD(scale)
    lt = np.asarray(log_trans, dtype=np.float32).astype(np.float64)
    li = np.asarray(log_init, dtype=np.float32).astype(np.float64)
    g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(np.float64)
    covers = []                                             # (total, moves): (start, 0, -1) or (start, d, k)

    def walk(n, total, moves, last):
        if n == N:
            covers.append((total, moves))
            return
        if g is not None and g[n] > NEG:
            walk(n + 1, total + LD(g[n]) * s, moves + [(n, 0, -1)], last)
        for d in range(d_min, min(D, N - n) + 1):
            for k in range(K):
                link = li[k] if last < 0 else lt[last, k]
                w = T[n + d, d - 1, k]
                if w > NEG and link > NEG:
                    walk(n + d, total + (LD(w) + LD(link) + LD(seg_bonus)) * s, moves + [(n, d, k)], k)
    with np.errstate(invalid="ignore"):
        walk(0, LD(0.0), [], -1)
    post_k = np.zeros((2, N + 1, K), dtype=LD)
    gap_post = np.zeros(N + 1, dtype=LD)
    tc, ic = np.zeros((K, K), dtype=LD), np.zeros(K, dtype=LD)
    span = np.zeros((N + 1, D), dtype=LD)
    no_seg = LD(0)
    f = np.float64
    if not covers:
        return dict(log_z=NEG, post_k=post_k.astype(f), gap_post=gap_post.astype(f), trans_counts=tc.astype(f),
                    init_counts=ic.astype(f), span_post=span.astype(f), no_segment=0.0)
    m = max(t for t, _ in covers)
    z = sum(np.exp(t - m) for t, _ in covers)
    for t, moves in covers:
        p = np.exp(t - m) / z
        last = -1
        for st, d, k in moves:
            if d == 0:
                gap_post[st] += p
                continue
            post_k[0, st, k] += p
            post_k[1, st + d, k] += p
            span[st + d, d - 1] += p
            if last < 0:
                ic[k] += p
            else:
                tc[last, k] += p
            last = k
        if last < 0:
            no_seg += p
    return dict(log_z=float(m + np.log(z)), post_k=post_k.astype(f), gap_post=gap_post.astype(f),
                trans_counts=tc.astype(f), init_counts=ic.astype(f), span_post=span.astype(f),
                no_segment=float(no_seg))


def lattice_bar(N, D, K, lattice):
    """8 N (D + K + 2) 2^-53 (M + 1), M the largest finite |value| of the reference lattice (doubled when the
    reference itself is float64)."""
    lattice = np.asarray(lattice)
    fin = np.abs(lattice[np.isfinite(lattice)])
    M = float(fin.max()) if fin.size else 0.0
    return (1 if LD_OK else 2) * 8.0 * max(N, 1) * (D + K + 2) * 2.0 ** -53 * (M + 1.0)


def identities(r, with_table=True):
    """The worst absolute violations of identities (i)-(v) of the issue on a
    result dict (the reference's, or the device's outputs under the same
    keys): dict(cover, ends, onsets, init, trans).  Where log_z = -inf
    everything is zero and only the zero sums are compared."""
    on, en = np.asarray(r["post_k"][0]), np.asarray(r["post_k"][1])
    N = on.shape[0] - 1
    lz = r["log_z"]
    G, aW = r["lattice_g"][0], r["lattice"][2]
    reach = lz > NEG
    out = {}
    inside = np.cumsum((on - en).sum(1))[:N]
    out["cover"] = float(np.abs(r["gap_post"][:N] + inside - 1.0).max()) if (N and reach) else 0.0
    if with_table:
        out["ends"] = float(np.abs(r["span_post"].sum(1) - en.sum(1)).max())
    tc, ic = r["trans_counts"], r["init_counts"]
    out["onsets"] = float(np.abs(tc.sum(0) + ic - on.sum(0)).max())
    with np.errstate(invalid="ignore", over="ignore"):
        none = float(np.exp(G[N] - lz)) if reach and G[N] > NEG else 0.0
        last = np.where(aW[N] > NEG, np.exp(np.where(aW[N] > NEG, aW[N], 0) - lz), 0.0) if reach else np.zeros(len(ic))
    out["init"] = abs(float(ic.sum()) - (1.0 - none)) if reach else abs(float(ic.sum()))
    out["trans"] = float(np.abs(tc.sum(1) - (en.sum(0) - last)).max())
    return out


@functools.lru_cache(maxsize=None)
def reference_of(N, D, K, kind, call, init_none=False, scale=1.0):
    """chain_posterior_reference on call ``call`` of syntax_cases.chain_inputs(N, D, K, kind); shared, never
    modified."""
    c = SX.chain_inputs(N, D, K, kind)
    d_min, gap, bonus, _ = c["calls"][call]
    return chain_posterior_reference(c["table"], d_min, c["trans"], c["init_none"] if init_none else c["init"], gap,
                                     bonus, scale)


# ----------------------------------------------------------------------------
# EM on uncut recordings
# ----------------------------------------------------------------------------
EM_SHAPE = (33, 5, 3)          # N, D, K
EM_RECORDINGS, EM_ITERS = 3, 6


@functools.lru_cache(maxsize=None)
def em_recordings(N=EM_SHAPE[0], D=EM_SHAPE[1], K=EM_SHAPE[2], count=EM_RECORDINGS):
    """``count`` drawn recordings: (table, gap) each, N(0, 3) tables and a drawn gap."""
    g = np.random.default_rng(7919 * N + 13 * D + K)
    return tuple((SX.random_table(g, N, D, K), g.normal(-1.0, 1.0, size=N).astype(np.float32)) for _ in range(count))


def m_step(tc, ic, c, old_t, old_i):
    """(log_trans, log_init) in fp32 from the counts: (counts + c) normalised per row, a zero row kept."""
    t, i = np.asarray(tc, dtype=np.float64) + c, np.asarray(ic, dtype=np.float64) + c
    rs = t.sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        trans = np.where(rs > 0, t / np.maximum(rs, 1e-300), np.exp(old_t.astype(np.float64)))
        init = i / i.sum() if i.sum() > 0 else np.exp(old_i.astype(np.float64))
        return np.log(trans).astype(np.float32), np.log(init).astype(np.float32)


def em_objective(evidence, lt, li, c, temperature):
    lt, li = np.asarray(lt, dtype=np.float64), np.asarray(li, dtype=np.float64)
    return temperature * evidence + c * (lt[np.isfinite(lt)].sum() + li[np.isfinite(li)].sum())


def em_reference(recordings, K, d_min, n_iter, c, temperature=1.0, seg_bonus=0.0):
    """Baum-Welch on uncut recordings by the reference: dict(objectives (n_iter
    + 1: before each iteration and after the last), evidence (the summed log
    evidence beside each), L (the largest finite |log-probability| visited),
    M (the largest finite |value| of any lattice), trans, init)."""
    lt = np.full((K, K), -np.log(K), dtype=np.float32)
    li = np.full(K, -np.log(K), dtype=np.float32)
    objs, evs, L, M = [], [], 0.0, 0.0
    for it in range(n_iter + 1):
        tc, ic, ev = np.zeros((K, K)), np.zeros(K), 0.0
        for table, gap in recordings:
            r = chain_posterior_reference(table, d_min, lt, li, gap, seg_bonus, 1.0 / temperature, want_table=False)
            ev += r["log_z"]
            M = max(M, float(np.abs(r["lattice"][np.isfinite(r["lattice"])]).max()))
            tc += r["trans_counts"]
            ic += r["init_counts"]
        objs.append(float(em_objective(ev, lt, li, c, temperature)))
        evs.append(ev)
        L = max([L] + [float(np.abs(v[np.isfinite(v)]).max()) for v in (lt, li) if np.isfinite(v).any()])
        if it < n_iter:
            lt, li = m_step(tc, ic, c, lt, li)
    return dict(objectives=objs, evidence=evs, L=L, M=M, trans=lt, init=li)


def em_slack(L, recordings, d_min, c, K):
    """2^-23 L (sum N / d_min + c (K^2 + K)): the fp32 rounding of the stored parameters, one rounding of relative
    size 2^-24 (2^-23 taken) per log-probability a cover can pay and per penalty term."""
    total = sum(t.shape[0] - 1 for t, _ in recordings)
    return 2.0 ** -23 * L * (total / d_min + c * (K * K + K))


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as spanpost_cases.dump)."""
    PC.PW.E.dump_observed("chainpost_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/chainpost_errors.json from a run of tests/test_gpu_chainpost.py
    with ABCD_PARITY_DUMP=<dump_dir>: the worst error over its bar per group."""
    import glob
    import json
    import os
    groups = {}
    for kind in ("sweep", "width", "reduction", "em", "e2e"):
        rows = []
        for path in sorted(glob.glob(os.path.join(dump_dir, f"chainpost_{kind}_*.json"))):
            with open(path) as f:
                rows += json.load(f)
        groups[kind] = rows
    keys = ("lattice_over_bar", "log_z_over_bar", "post_over_bar", "counts_over_bar", "span_over_bar",
            "identities_over_bar", "bg0_over_bar")
    worst = {k: max((r[k] for rows in (groups["sweep"], groups["width"]) for r in rows if k in r), default=None)
             for k in keys}
    worst["reduction_over_bar"] = max((r["over_bar"] for r in groups["reduction"]), default=None)
    worst["em_objective_over_bar"] = max((r["over_bar"] for r in groups["em"]), default=None)
    doc = dict(what="figures observed by tests/test_gpu_chainpost.py (ABCD_PARITY_DUMP) on one MI355X; units and "
                    "bars: tests/chainpost_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(lattice="8 N (D + K + 2) 2^-53 (M + 1)", posterior="5 lattice bars",
                         counts="5 lattice bars (1 + reference)", identities="5 lattice bars, times N for the summed"),
               worst=worst, **groups)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/chainpost_cases.py <dump directory> <out.json> <date> <parent commit>
    import sys
    print(assemble(*sys.argv[1:5])["worst"])
