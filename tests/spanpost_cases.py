"""References of the segmentation posteriors: the span scores summed over the
categories (``abcd_span_evidence``) and the semi-Markov forward-backward over a
span table (``abcd_span_posterior``, ``modules.segmentation.segment_posteriors``,
``segment.py --posteriors``).

``span_cases`` supplies the inputs and the float64 ``S`` / ``A`` of every
(start, prototype, length); it is imported and left as it is.  The programme's
reference runs the recursions of DESIGN s3.12 in ``np.longdouble`` and is itself
checked against brute-force enumeration of every cover (test_spanpost_cpu.py).

Bars.  ``span_lse`` within ``BAR`` (1e-4, the project's bar for S) of the unit
``max_p A`` of the entry's admissible prototypes.  The lattice (alpha,
alpha_seg, beta, beta_seg) within ``lattice_bar``: 8 N (D + 2) 2^-53 (M + 1)
absolute, M the largest finite |value| of the reference lattice -- a rounding
per combine and a few ulp of libm, at most D combines per step, errors passed
from step to step with weight <= 1.  Posteriors within 5 lattice bars,
absolute."""
import functools

import numpy as np

import pairwise_cases as PW
import span_cases as SP

NEG = -np.inf
BAR = SP.BAR
LD = np.longdouble
LD_OK = np.finfo(LD).eps < 1e-18
"""x87 extended or better; otherwise the reference runs in float64 and the lattice bar is doubled."""

EV_SHAPES = ((1, 1), (33, 5), (33, 37), (70, 16), (70, 17))
EV_P = (1, 17, 33, 65)
EV_F = (1, 65)

POST_N = (0, 1, 2, 33, 300)
POST_D = (1, 5, 64, 65, 256, 257, 300)
KINDS = ("random", "tied", "holes")


def lse_reference(S):
    """span_lse (N + 1 x D float64, end-major) from span_reference's S (N x P
    x D): the log-sum over the prototypes whose S is neither NaN nor -inf; -inf
    where nothing is left or d > e."""
    S = np.asarray(S, dtype=np.float64)
    N, _, D = S.shape
    out = np.full((N + 1, D), NEG)
    for e in range(1, N + 1):
        for d in range(1, min(D, e) + 1):
            s = S[e - d, :, d - 1]
            with np.errstate(invalid="ignore"):
                ok = s > NEG
            if ok.any():
                v = s[ok].astype(LD)
                m = v.max()
                out[e, d - 1] = float(m + np.log(np.exp(v - m).sum()))
    return out


def unit_reference(S, A):
    """max_p A over the admissible prototypes of each entry (N + 1 x D; NaN where there is none)."""
    S, A = np.asarray(S), np.asarray(A)
    N, _, D = S.shape
    out = np.full((N + 1, D), np.nan)
    for e in range(1, N + 1):
        for d in range(1, min(D, e) + 1):
            with np.errstate(invalid="ignore"):
                ok = S[e - d, :, d - 1] > NEG
            if ok.any():
                out[e, d - 1] = A[e - d, ok, d - 1].max()
    return out


def _lse(values):
    """log-sum-exp of the candidates above -inf (NaN excluded); -inf over none."""
    v = [c for c in values if c > NEG]
    if not v:
        return LD(NEG)
    m = max(v)
    return m + np.log(sum(np.exp(c - m) for c in v))


def posterior_reference(span, d_min, gap=None, seg_bonus=0.0, dtype=None):
    """The recursions of the issue in np.longdouble: dict(log_z, lattice (4 x
    (N + 1)), post (3 x (N + 1)), span_post (N + 1 x D)), float64 each.  gap is
    rounded to fp32 first, as the kernel reads it."""
    T = dtype or (LD if LD_OK else np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        W = np.asarray(span, dtype=np.float64).astype(T)
        N, D = W.shape[0] - 1, W.shape[1]
        g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(T)
        bonus = T(seg_bonus)
        neg = T(NEG)
        a, aseg = np.full(N + 1, neg), np.full(N + 1, neg)
        b, bseg = np.full(N + 1, neg), np.full(N + 1, neg)
        a[0] = 0
        for n in range(1, N + 1):
            aseg[n] = bonus + _lse([a[n - d] + W[n, d - 1] for d in range(d_min, min(D, n) + 1)])
            a[n] = _lse([a[n - 1] + g[n - 1] if g is not None else neg, aseg[n]])
        b[N] = 0
        for n in range(N - 1, -1, -1):
            bseg[n] = _lse([W[n + d, d - 1] + bonus + b[n + d] for d in range(d_min, min(D, N - n) + 1)])
            b[n] = _lse([g[n] + b[n + 1] if g is not None else neg, bseg[n]])
        lz = a[N]
        post = np.zeros((3, N + 1), dtype=T)
        table = np.zeros((N + 1, D), dtype=T)
        if lz > NEG:
            for n in range(N + 1):
                if n < N:
                    post[0, n] = np.exp(a[n] + bseg[n] - lz)
                    if g is not None:
                        post[2, n] = np.exp(a[n] + g[n] + b[n + 1] - lz)
                if n >= 1:
                    post[1, n] = np.exp(aseg[n] + b[n] - lz)
            for e in range(1, N + 1):
                for d in range(d_min, min(D, e) + 1):
                    c = a[e - d] + W[e, d - 1] + bonus + b[e]
                    if c > NEG:
                        table[e, d - 1] = np.exp(c - lz)
        post = np.where(np.isnan(post), 0, post)
    return dict(log_z=float(lz), lattice=np.stack([a, aseg, b, bseg]).astype(np.float64),
                post=post.astype(np.float64), span_post=table.astype(np.float64))


def posterior_reference_fast(span, d_min, gap=None, seg_bonus=0.0):
    """posterior_reference with each step's candidates as one numpy vector (the
    same recursions and precision; for the larger GPU cases)."""
    T = LD if LD_OK else np.float64
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        W = np.asarray(span, dtype=np.float64).astype(T)
        N, D = W.shape[0] - 1, W.shape[1]
        g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(T)
        bonus, neg = T(seg_bonus), T(NEG)

        def lse(c):
            c = c[c > NEG]
            if not c.size:
                return neg
            m = c.max()
            return m + np.log(np.exp(c - m).sum())

        a, aseg = np.full(N + 1, neg), np.full(N + 1, neg)
        b, bseg = np.full(N + 1, neg), np.full(N + 1, neg)
        a[0] = 0
        for n in range(1, N + 1):
            hi = min(D, n)
            if hi >= d_min:
                aseg[n] = bonus + lse(a[n - hi:n - d_min + 1][::-1] + W[n, d_min - 1:hi])
            a[n] = lse(np.array([a[n - 1] + g[n - 1] if g is not None else neg, aseg[n]]))
        b[N] = 0
        ix = np.arange(D)
        for n in range(N - 1, -1, -1):
            hi = min(D, N - n)
            if hi >= d_min:
                d = ix[d_min - 1:hi]                       # d - 1
                bseg[n] = lse(W[n + d + 1, d] + bonus + b[n + d + 1])
            b[n] = lse(np.array([g[n] + b[n + 1] if g is not None else neg, bseg[n]]))
        lz = a[N]
        post = np.zeros((3, N + 1), dtype=T)
        table = np.zeros((N + 1, D), dtype=T)
        if lz > NEG:
            post[0, :N] = np.exp(a[:N] + bseg[:N] - lz)
            post[1, 1:] = np.exp(aseg[1:] + b[1:] - lz)
            if g is not None:
                post[2, :N] = np.exp(a[:N] + g + b[1:] - lz)
            for e in range(1, N + 1):
                hi = min(D, e)
                if hi >= d_min:
                    c = a[e - hi:e - d_min + 1][::-1] + W[e, d_min - 1:hi] + bonus + b[e]
                    table[e, d_min - 1:hi] = np.where(c > NEG, np.exp(c - lz), 0)
        post = np.where(np.isnan(post), 0, post)
    return dict(log_z=float(lz), lattice=np.stack([a, aseg, b, bseg]).astype(np.float64),
                post=post.astype(np.float64), span_post=table.astype(np.float64))


def brute_force_posterior(span, d_min, gap=None, seg_bonus=0.0):
    """Every cover of N <= 9 frames enumerated: dict(log_z, post (3 x (N + 1)),
    span_post (N + 1 x D)) from the covers' weights, in np.longdouble."""
    W = np.asarray(span, dtype=np.float64)
    N, D = W.shape[0] - 1, W.shape[1]
    assert N <= 9
    g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(np.float64)
    covers = []                                         # (total, moves): a move is (start, 0) or (start, d)

    def walk(n, total, moves):
        if n == N:
            covers.append((total, moves))
            return
        if g is not None and g[n] > NEG:
            walk(n + 1, total + LD(g[n]), moves + [(n, 0)])
        for d in range(d_min, min(D, N - n) + 1):
            w = W[n + d, d - 1]
            if w > NEG:
                walk(n + d, total + LD(w) + LD(seg_bonus), moves + [(n, d)])
    with np.errstate(invalid="ignore"):
        walk(0, LD(0.0), [])
    post = np.zeros((3, N + 1), dtype=LD)
    table = np.zeros((N + 1, D), dtype=LD)
    if not covers:
        return dict(log_z=NEG, post=post.astype(np.float64), span_post=table.astype(np.float64))
    m = max(t for t, _ in covers)
    z = sum(np.exp(t - m) for t, _ in covers)
    for t, moves in covers:
        p = np.exp(t - m) / z
        for s, d in moves:
            if d == 0:
                post[2, s] += p
            else:
                post[0, s] += p
                post[1, s + d] += p
                table[s + d, d - 1] += p
    return dict(log_z=float(m + np.log(z)), post=post.astype(np.float64), span_post=table.astype(np.float64))


def lattice_bar(N, D, lattice):
    """8 N (D + 2) 2^-53 (M + 1), M the largest finite |value| of the reference lattice (doubled when the
    reference itself is float64)."""
    fin = np.abs(lattice[np.isfinite(lattice)])
    M = float(fin.max()) if fin.size else 0.0
    return (1 if LD_OK else 2) * 8.0 * max(N, 1) * (D + 2) * 2.0 ** -53 * (M + 1.0)


def identities(post, span_post, with_gap):
    """The four identities' worst absolute violations: dict(cover (gap_post[n]
    + the span posteriors covering n = 1; only where the recording can be
    covered), ends, onsets)."""
    N, D = span_post.shape[0] - 1, span_post.shape[1]
    e, d = np.arange(N + 1)[:, None], np.arange(1, D + 1)[None, :]
    valid = d <= e
    start, end, p = (e - d)[valid], np.broadcast_to(e, valid.shape)[valid], np.asarray(span_post)[valid]
    step = np.zeros(N + 1)                              # the spans covering n: those started minus those ended by n
    np.add.at(step, start, p)
    np.add.at(step, end, -p)
    cover = np.asarray(post[2][:N], dtype=np.float64) + np.cumsum(step)[:N]
    ends = np.abs(span_post.sum(1) - post[1]).max()
    on = np.zeros(N + 1)
    np.add.at(on, start, p)
    return dict(cover=float(np.abs(cover - 1.0).max()) if N else 0.0, ends=float(ends),
                onsets=float(np.abs(on - post[0]).max()))


@functools.lru_cache(maxsize=None)
def evidence_case(N, D, P, F):
    """span_cases.abi_inputs with the lse reference and its unit beside it (shared, never modified)."""
    c = SP.abi_inputs(N, D, P, F)
    return dict(c, lse=lse_reference(c["ref"]["S"]), unit=unit_reference(c["ref"]["S"], c["ref"]["A"]))


@functools.lru_cache(maxsize=None)
def tail_posterior(name, with_gap):
    """posterior_reference_fast on span_cases.tail_inputs(name), bonus 0 (shared, never modified)."""
    t = SP.tail_inputs(name)
    return posterior_reference_fast(t["score"], t["d_min"], t["gap"] if with_gap else None, 0.0)


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    PW.E.dump_observed("spanpost_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/spanpost_errors.json from a run of tests/test_gpu_spanpost.py
    with ABCD_PARITY_DUMP=<dump_dir>."""
    import glob
    import json
    import os
    groups = {}
    for kind in ("evidence", "identical", "posterior", "kernel", "order", "planted", "e2e"):
        rows = []
        for path in sorted(glob.glob(os.path.join(dump_dir, f"spanpost_{kind}_*.json"))):
            with open(path) as f:
                rows += json.load(f)
        groups[kind] = rows
    worst = dict(evidence_lse_over_unit=max((r["lse"] for r in groups["evidence"]), default=None),
                 identical_log_p=max((r["err"] for r in groups["identical"]), default=None),
                 posterior_lattice_over_bar=max((r["lattice_over_bar"] for r in groups["posterior"]), default=None),
                 posterior_post_over_bar=max((r["post_over_bar"] for r in groups["posterior"]), default=None),
                 kernel_lattice_over_bar=max((r["lattice_over_bar"] for r in groups["kernel"]), default=None))
    doc = dict(what="figures observed by tests/test_gpu_spanpost.py (ABCD_PARITY_DUMP) on one MI355X; units and "
                    "bars: tests/spanpost_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(span_lse=BAR, identical_log_p=1e-6, lattice="8 N (D + 2) 2^-53 (M + 1)",
                         posterior="5 lattice bars"), worst=worst, **groups)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/spanpost_cases.py <dump directory> <out.json> <date> <parent commit>
    import sys
    print(assemble(*sys.argv[1:5])["worst"])
