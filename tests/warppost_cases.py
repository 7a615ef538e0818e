"""Cases, references and bars of the posteriors under the time-warped cut: the
forward-backward over (frame, category k, prototype step s)
(``abcd_warp_posterior_forward`` / ``abcd_warp_posterior_backward``,
``ops.warp_posterior_forward`` / ``ops.warp_posterior_backward``,
``segmentation.segment_warp_posteriors`` / ``refit_warp_em``, ``segment.py --warp
--warp_posteriors`` / ``--warp_refit``).  ``warpseg_cases``
supplies the inputs (``prog_inputs``), ``chainpost_cases`` the rigid reference
the step-only programme is checked against and its longdouble helpers, and
``syntax_cases`` is what both build on; all three are imported and left as they
are.

The recursions, in ``np.longdouble``.  e, cont, last, lm, le, gap, bonus, lt, li
are the inputs (fp32 ones widened) times ``scale``, cont = sp(v) and last = sp(-v)
formed before the multiplication; a candidate that is NaN or -inf is excluded, a
NaN or +inf e excludes its cell in both sweeps; LAE is logaddexp, LSE the
log-sum-exp, -inf over none; T is the number of prototype steps:

    G[0] = 0;  G[n] = G[n-1] + gap[n-1]                    (gap None: -inf for n >= 1)
    aW[0][k] = -inf;  aH[-1] = -inf
    aU[n][k]    = LAE(G[n] + li[k], LSE_k' (aW[n][k'] + lt[k'][k]))
    aA[n][0][k] = LAE(aU[n][k] + le[k], aH[n-1][0][k] + lm[0])
    aA[n][s][k] = LSE_{m, s-m >= 0} (aH[n-1][s-m][k] + lm[m])                  s >= 1
    aB = aA - e;  aH[n] = aB - cont
    aX[n+1][k]  = LSE_{s >= s_min} (aB[n][s][k] - last[s,k]) + bonus
    aW[n+1][k]  = LAE(aW[n][k] + gap[n], aX[n+1][k])
    aU[N] = -inf;  aX[0] = -inf;  log_z = LAE(G[N], LSE_k aW[N][k])
    bW[N] = 0, bG[N] = 0, bU[N] = -inf;  n = N-1 .. 0:
    bA[n][s][k] = -e + LAE([s >= s_min] (-last + bonus + bW[n+1][k]),
                           [n < N-1] (-cont + LSE_{m, s+m < T} (lm[m] + bA[n+1][s+m][k])))
    bU[n][k] = le[k] + bA[n][0][k]
    bW[n][k] = LAE(gap[n] + bW[n+1][k], LSE_k'' (lt[k][k''] + bU[n][k'']))
    bG[n]    = LAE(gap[n] + bG[n+1], LSE_k (li[k] + bU[n][k]))

and the posteriors and counts of DESIGN.md s3.17 from them.

Bars (chainpost_cases' formulas carried over, not tuned).  A step has K + 1
candidates in U, at most 4 in A, T in X and 2 in W, so the lattice is within
``lattice_bar``: 8 N (T + K + 8) 2^-53 (M + 1) absolute, M the largest finite
|value| of the reference lattice, doubled when longdouble is not extended
precision.  Posteriors within 5 lattice bars absolute, a count entry within 5
lattice bars times (1 + its reference value), cont / last within
``warpseg_cases.SP_ULPS`` ulps of numpy's.

Shapes: warpseg_cases' own.  The plan has no launch-width threshold (1024 threads
at every K), so no K = 256 / 257 pair is added; K = 130 is the streamed matrix."""
import functools
import glob
import json
import os

import numpy as np

import chainpost_cases as CP
import syntax_cases as SX  # noqa: F401  (the cases this file's inputs come from)
import warpseg_cases as WS

NEG = -np.inf
LD_OK = CP.LD_OK
RT = CP.RT
MOVES = WS.MOVES
SP_ULPS = WS.SP_ULPS
PAD_LD = WS.PAD_LD

PROG_N = WS.PROG_N
PROG_KT = WS.PROG_KT
PROG_KINDS = WS.PROG_KINDS
PROG_SMIN = WS.PROG_SMIN
SCALES = (1.0, 0.25)

_f32, _clean, _lse, _lae = CP._f32, CP._clean, CP._lse, CP._lae


def _ex(c):
    return np.where(c > NEG, np.exp(np.where(c > NEG, c, 0)), 0)


def warp_posterior_reference(cost, v, log_move, log_enter, gap, seg_bonus, log_trans, log_init, s_min=0, scale=1.0,
                             cont=None, last=None):
    """The recursions above, each frame's candidates as one numpy array (the
    sums over k' through E = exp(lt), as chainpost_cases does).  cost is N x T x
    K (or N x T K), v is T x K; cont / last (T x K float64, unscaled) replace
    numpy's sp(v) / sp(-v) when given.  dict of float64 arrays log_z, lattice (5
    x (N + 1) x K: aU, aX, aW, bU, bW), lattice_g (2 x (N + 1): G, bG), post_k (2
    x (N + 1) x K: onset, end), gap_post (N + 1), trans_counts (K x K),
    init_counts (K), move_counts (K x 3) and no_segment."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s = RT(scale)
        v32 = np.asarray(v, dtype=np.float32).astype(np.float64)
        T, K = v32.shape
        raw = np.asarray(cost, dtype=np.float32).astype(np.float64).reshape(-1, T, K)
        N = raw.shape[0]
        bad = ~(raw < np.inf)                                                   # NaN or +inf
        e = np.where(bad, 0.0, raw).astype(RT) * s
        cont = (WS.softplus(v32) if cont is None else np.asarray(cont, dtype=np.float64).reshape(T, K)).astype(RT) * s
        last = (WS.softplus(-v32) if last is None else np.asarray(last, dtype=np.float64).reshape(T, K)).astype(RT) * s
        lm = [RT(float(m)) * s for m in log_move]
        le = np.zeros(K, dtype=RT) if log_enter is None else _f32(log_enter) * s
        lt, li = _f32(log_trans) * s, _f32(log_init) * s
        g = None if gap is None else _f32(gap) * s
        bonus, neg = RT(seg_bonus) * s, RT(NEG)
        E = np.exp(_clean(lt))

        def through(vec, into):
            vec = _clean(vec)
            m = vec.max()
            if not m > NEG:
                return np.full(K, neg)
            w = np.exp(vec - m)
            z = w @ E if into else E @ w
            return np.where(z > 0, m + np.log(np.where(z > 0, z, 1)), neg)

        G = np.full(N + 1, neg)
        G[0] = 0
        aU, aX, aW, bU, bW = (np.full((N + 1, K), neg) for _ in range(5))
        bG = np.full(N + 1, neg)
        aH = np.full((N, T, K), neg)
        H = np.full((T, K), neg)
        for n in range(N):
            aU[n] = _lae(G[n] + li, through(aW[n], True))
            cand = np.full((4, T, K), neg)
            cand[0, 0] = aU[n] + le
            cand[1] = H + lm[0]
            if T > 1:
                cand[2, 1:] = H[:-1] + lm[1]
            if T > 2:
                cand[3, 2:] = H[:-2] + lm[2]
            aB = np.where(bad[n], neg, _clean(_lse(cand, 0) - e[n]))
            H = _clean(aB - cont)
            aH[n] = H
            xc = aB - last
            xc[:s_min] = neg
            aX[n + 1] = _clean(_lse(xc, 0) + bonus)
            gv = g[n] if g is not None else neg
            G[n + 1] = G[n] + gv
            aW[n + 1] = _lae(aW[n] + gv, aX[n + 1])
        lz = _lae(G[N], _lse(aW[N], 0)) if N > 0 else RT(0)
        reach = bool(lz > NEG)
        bW[N], bG[N] = 0, 0
        mc = np.zeros((K, 3), dtype=RT)
        B = None
        for n in range(N - 1, -1, -1):
            gv = g[n] if g is not None else neg
            endc = np.full((T, K), neg)
            endc[s_min:] = (bonus - last[s_min:]) + bW[n + 1][None, :]
            contc = np.full((T, K), neg)
            if n < N - 1:
                c = np.full((3, T, K), neg)
                c[0] = lm[0] + B
                if T > 1:
                    c[1, :-1] = lm[1] + B[1:]
                if T > 2:
                    c[2, :-2] = lm[2] + B[2:]
                contc = _clean(_lse(c, 0) - cont)
                if reach:
                    for m in range(3):
                        if T > m:
                            mc[:, m] += _ex(aH[n][:T - m] + lm[m] + B[m:] - lz).sum(0)
            B = np.where(bad[n], neg, _clean(_lae(endc, contc) - e[n]))
            bU[n] = _clean(le + B[0])
            bW[n] = _lae(gv + bW[n + 1], through(bU[n], False))
            bG[n] = _lae(gv + bG[n + 1], _lse(li + bU[n], 0))
        post_k = np.zeros((2, N + 1, K), dtype=RT)
        gap_post = np.zeros(N + 1, dtype=RT)
        tc, ic = np.zeros((K, K), dtype=RT), np.zeros(K, dtype=RT)
        no_seg = RT(0)
        if reach and N > 0:
            post_k[0] = _ex(aU + bU - lz)
            post_k[1] = _ex(aX + bW - lz)
            if g is not None:
                inner = _lae(G[:N] + bG[1:], _lse(aW[:N] + bW[1:], 1))
                gap_post[:N] = _ex(inner + g - lz)
            for n in range(N):
                ic += _ex(G[n] + li + bU[n] - lz)
                a, b = _clean(aW[n]), _clean(bU[n])
                ma, mb = a.max(), b.max()
                if ma > NEG and mb > NEG:
                    tc += (np.exp(a - ma)[:, None] * E * np.exp(b - mb)[None, :]) * np.exp(ma + mb - lz)
            no_seg = _ex(G[N] - lz)
        elif N == 0:
            no_seg = RT(1)
        f = np.float64
        return dict(log_z=float(lz), lattice=np.stack([aU, aX, aW, bU, bW]).astype(f),
                    lattice_g=np.stack([G, bG]).astype(f), post_k=post_k.astype(f), gap_post=gap_post.astype(f),
                    trans_counts=tc.astype(f), init_counts=ic.astype(f), move_counts=mc.astype(f),
                    no_segment=float(no_seg))


def enumerate_covers(cost, v, log_move, log_enter, gap, seg_bonus, log_trans, log_init, s_min=0, scale=1.0):
    """Every cover by gap frames and segments, every labelling and every move
    sequence of a tiny case (N <= 4, K <= 2, T <= 3), each path's weight added
    as written in np.longdouble: dict of log_z, post_k, gap_post, trans_counts,
    init_counts, move_counts, no_segment and paths (how many), all from the
    paths' weights alone."""
    LD = CP.LD
    v32 = np.asarray(v, dtype=np.float32).astype(np.float64)
    T, K = v32.shape
    e = np.asarray(cost, dtype=np.float32).astype(np.float64).reshape(-1, T, K)
    N = e.shape[0]
    assert N <= 4 and K <= 2 and T <= 3
    s = LD(scale)
    lm = [float(m) for m in log_move]
    le = np.zeros(K) if log_enter is None else np.asarray(log_enter, dtype=np.float32).astype(np.float64)
    lt = np.asarray(log_trans, dtype=np.float32).astype(np.float64)
    li = np.asarray(log_init, dtype=np.float32).astype(np.float64)
    g = None if gap is None else np.asarray(gap, dtype=np.float32).astype(np.float64)
    cont, last = WS.softplus(v32), WS.softplus(-v32)
    paths = []                                               # (total, events)

    def ok(x):
        return x > NEG                                       # False for NaN

    def inside(n, k, st, total, ev):
        if not (e[n, st, k] < np.inf):
            return
        total = total - LD(e[n, st, k]) * s
        if st >= s_min:
            outside(n + 1, k, total - LD(last[st, k]) * s + LD(seg_bonus) * s, ev + [("end", n + 1, k)])
        if n + 1 < N:
            for m in range(3):
                if ok(lm[m]) and st + m < T:
                    inside(n + 1, k, st + m, total - LD(cont[st, k]) * s + LD(lm[m]) * s, ev + [("move", k, m)])

    def outside(n, kp, total, ev):
        if n == N:
            paths.append((total, ev, kp))
            return
        if g is not None and ok(g[n]):
            outside(n + 1, kp, total + LD(g[n]) * s, ev + [("gap", n)])
        for k in range(K):
            link = li[k] if kp < 0 else lt[kp, k]
            if ok(link) and ok(le[k]):
                inside(n, k, 0, total + LD(link) * s + LD(le[k]) * s,
                       ev + [("on", n, k), ("init", k) if kp < 0 else ("trans", kp, k)])

    outside(0, -1, LD(0.0), [])
    post_k = np.zeros((2, N + 1, K), dtype=LD)
    gap_post = np.zeros(N + 1, dtype=LD)
    tc, ic, mc = np.zeros((K, K), dtype=LD), np.zeros(K, dtype=LD), np.zeros((K, 3), dtype=LD)
    no_seg = LD(0)
    f = np.float64
    if not paths:
        return dict(log_z=NEG, post_k=post_k.astype(f), gap_post=gap_post.astype(f), trans_counts=tc.astype(f),
                    init_counts=ic.astype(f), move_counts=mc.astype(f), no_segment=0.0, paths=0)
    top = max(t for t, _, _ in paths)
    z = sum(np.exp(t - top) for t, _, _ in paths)
    for t, ev, kp in paths:
        p = np.exp(t - top) / z
        for item in ev:
            if item[0] == "on":
                post_k[0, item[1], item[2]] += p
            elif item[0] == "end":
                post_k[1, item[1], item[2]] += p
            elif item[0] == "gap":
                gap_post[item[1]] += p
            elif item[0] == "init":
                ic[item[1]] += p
            elif item[0] == "trans":
                tc[item[1], item[2]] += p
            else:
                mc[item[1], item[2]] += p
        if kp < 0:
            no_seg += p
    return dict(log_z=float(top + np.log(z)), post_k=post_k.astype(f), gap_post=gap_post.astype(f),
                trans_counts=tc.astype(f), init_counts=ic.astype(f), move_counts=mc.astype(f),
                no_segment=float(no_seg), paths=len(paths))


def lattice_bar(N, K, T, lattice):
    """8 N (T + K + 8) 2^-53 (M + 1), M the largest finite |value| of the reference lattice (doubled when the
    reference itself is float64)."""
    lattice = np.asarray(lattice)
    fin = np.abs(lattice[np.isfinite(lattice)])
    M = float(fin.max()) if fin.size else 0.0
    return (1 if LD_OK else 2) * 8.0 * max(N, 1) * (T + K + 8) * 2.0 ** -53 * (M + 1.0)


def identities(r):
    """The worst absolute violations of the four identities of DESIGN.md s3.17
    on a result dict: dict(bg0 (bG[0] against log_z), cover (per frame), onsets
    (sum onset = sum end = sum trans + sum init) and moves (sum moves + sum end
    = the covered frames)).  Where log_z = -inf everything is zero."""
    on, en = np.asarray(r["post_k"][0]), np.asarray(r["post_k"][1])
    N = on.shape[0] - 1
    lz = r["log_z"]
    reach = lz > NEG
    inside = np.cumsum(on - en, 0)[:N].sum(1)
    out = {}
    bg0 = r["lattice_g"][1][0]
    out["bg0"] = abs(float(bg0) - lz) if reach else (0.0 if not bg0 > NEG else np.inf)
    out["cover"] = float(np.abs(r["gap_post"][:N] + inside - 1.0).max()) if (N and reach) else 0.0
    links = float(r["trans_counts"].sum() + r["init_counts"].sum())
    out["onsets"] = max(abs(float(on.sum()) - float(en.sum())), abs(float(on.sum()) - links))
    out["moves"] = abs(float(r["move_counts"].sum()) + float(en.sum()) - float(inside.sum()))
    return out


def prog_reference(N, K, T, kind, moves, s_min, scale, cont=None, last=None):
    d = WS.prog_inputs(N, K, T, kind)
    return warp_posterior_reference(d["cost"], d["v"], MOVES[moves], d["enter"], d["gap"], d["bonus"], d["trans"],
                                    d["init"], s_min, scale, cont, last)


@functools.lru_cache(maxsize=None)
def reference_of(N, K, T, kind, moves, s_min, scale):
    """prog_reference on numpy's own sp planes; shared, never modified."""
    return prog_reference(N, K, T, kind, moves, s_min, scale)


def rigid_table64(cost, v, cont, last):
    """The float64 table the step-only programme equals the rigid one on, from the SAME plane and sp planes:
    T[e, d - 1, k] = -(sum_{t<d} e(e-d+t, t, k) + sum_{t<d-1} cont[t,k] + last[d-1,k]); -inf where d > e; a NaN or
    +inf cell makes its entries -inf."""
    v32 = np.asarray(v, dtype=np.float32)
    T, K = v32.shape
    e = np.asarray(cost, dtype=np.float32).astype(np.float64).reshape(-1, T, K)
    e = np.where(e < np.inf, e, np.inf)                      # NaN -> +inf: the entry becomes -inf
    N = e.shape[0]
    tab = np.full((N + 1, T, K), NEG)
    for end in range(1, N + 1):
        for d in range(1, min(T, end) + 1):
            tot = np.zeros(K)
            for t in range(d):
                tot = tot + e[end - d + t, t]
            tab[end, d - 1] = -(tot + cont[:d - 1].sum(0) + last[d - 1])
    return tab


# ----------------------------------------------------------------------------
# EM on a planted alternation
# ----------------------------------------------------------------------------
EM_ITERS = 4


@functools.lru_cache(maxsize=None)
def em_recordings():
    """Planes of two categories that alternate, every other segment played
    with its frames doubled: the planted state of a frame costs 0.5 under its
    segment's category and 2 under the other one, every other state 5, plus
    U[0, 0.25] per (frame, state).  A tuple of dict(cost (N x T K fp32), v (T x K
    fp32)) with K = 2, T = 3; uniform parameters do not know the alternation
    nor how often a frame stays."""
    g = np.random.default_rng(9973)
    T, K = 3, 2
    v = np.full((T, K), -2.0, dtype=np.float32)
    v[T - 1] = 2.0
    recs = []
    for r in range(3):
        states, cats = [], []
        for i in range(4 + r):
            path = [0, 1, 2] if i % 2 == 0 else [0, 0, 1, 1, 2, 2]
            states += path
            cats += [i % 2] * len(path)
        N = len(states)
        cost = np.full((N, T, K), 5.0, dtype=np.float32)
        for n, (st, k) in enumerate(zip(states, cats)):
            cost[n, st, k], cost[n, st, 1 - k] = 0.5, 2.0
        cost += g.random((N, T, 1)).astype(np.float32) * 0.25
        recs.append(dict(cost=cost.reshape(N, T * K), v=v))
    return tuple(recs)


def em_posterior_fn(log_enter=None, gap=None, seg_bonus=0.0, s_min=0):
    """``posterior_fn(recording, model, log_moves)`` for ``refit_warp_em`` by the reference."""
    def fn(rec, model, log_moves):
        if model is None:
            K = rec["v"].shape[1]
            lt, li = np.zeros((K, K), dtype=np.float32), np.zeros(K, dtype=np.float32)
        else:
            lt, li = model.log_trans.cpu().numpy(), model.log_init.cpu().numpy()
        r = warp_posterior_reference(rec["cost"], rec["v"], log_moves, log_enter, gap, seg_bonus, lt, li, s_min)
        return dict(log_evidence=r["log_z"], trans_counts=r["trans_counts"], init_counts=r["init_counts"],
                    move_counts=r["move_counts"], lattice=r["lattice"])
    return fn


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as chainpost_cases.dump)."""
    CP.PC.PW.E.dump_observed("warppost_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/warppost_errors.json from a run of tests/test_gpu_warppost.py
    with ABCD_PARITY_DUMP=<dump_dir>: per output the worst error over its bar,
    overall and per (N, K, T, kind) over that case's s_min and scale, one row
    per line."""
    groups = {}
    for kind in ("sweep", "rigid", "em", "e2e"):
        rows = []
        for path in sorted(glob.glob(os.path.join(dump_dir, f"warppost_{kind}_*.json"))):
            with open(path) as f:
                rows += json.load(f)
        groups[kind] = rows
    keys = ("sp_ulps", "lattice_over_bar", "log_z_over_bar", "post_over_bar", "gap_over_bar", "trans_over_bar",
            "init_over_bar", "moves_over_bar", "bg0_over_bar")
    worst = {k: max((r[k] for r in groups["sweep"] if k in r), default=None) for k in keys}
    worst["rigid_over_bar"] = max((r["over_bar"] for r in groups["rigid"]), default=None)
    worst["em_counts_over_bar"] = max((r["over_bar"] for r in groups["em"]), default=None)
    cases = {}
    for r in groups["sweep"]:
        c = cases.setdefault((r["N"], r["K"], r["T"], r["kind"]), dict(N=r["N"], K=r["K"], T=r["T"], kind=r["kind"],
                                                                       sweeps=0))
        c["sweeps"] += 1
        for k in keys:
            c[k] = float(f"{max(c.get(k, 0.0), r[k]):.3g}")
    groups["sweep"] = [cases[k] for k in sorted(cases)]
    head = dict(what="figures observed by tests/test_gpu_warppost.py (ABCD_PARITY_DUMP) on one MI355X; units and "
                     "bars: tests/warppost_cases.py", date=date, parent_commit=parent_commit,
                bars=dict(lattice="8 N (T + K + 8) 2^-53 (M + 1)", posterior="5 lattice bars",
                          counts="5 lattice bars (1 + reference)", sp_ulps=SP_ULPS), worst=worst)
    with open(out_path, "w") as f:
        f.write(json.dumps(head, indent=1)[:-2])
        for name, rows in groups.items():
            f.write(f',\n "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]")
        f.write("\n}\n")
    return dict(head, **groups)


if __name__ == "__main__":  # python tests/warppost_cases.py <dump directory> <out.json> <date> <parent commit>
    import sys
    print(assemble(*sys.argv[1:5])["worst"])
