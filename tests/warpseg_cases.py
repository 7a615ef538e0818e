"""Cases and the float64 references of time-warped segmentation
(``abcd_frame_costs``, ``abcd_warp_segment_window``, ``segment_frames_warped``,
``segment.py --warp``): DESIGN.md s3.16 in its written form.  ``span_cases``,
``syntax_cases`` and ``warp_cases`` are imported and left as they are.

The state is (category k, prototype step s).  On a plane e[n, s, k] (the
rectangle's row r = s K + k), in fp64 with every addition as written (fp32
inputs widened), sp(u) = max(u,0) + log1p(e^-|u|):

    cont[s,k] = sp(v[s,k])     last[s,k] = sp(-v[s,k])
    G[0] = 0;  G[n] = G[n-1] + gap[n-1]          (gap None: -inf for n >= 1)
    W[0][k] = -inf;  H[-1] = -inf
    U[n][k]    = max(G[n] + log_init[k], max_k' (W[n][k'] + log_trans[k'][k]))
    A[n][0][k] = max(U[n][k] + log_enter[k], H[n-1][0][k] + log_move[0])
    A[n][s][k] = max_{m, s-m >= 0} (H[n-1][s-m][k] + log_move[m])              s >= 1
    H[n][s][k] = (A[n][s][k] - e[n,s,k]) - cont[s,k]
    X[n+1][k]  = max_{s >= s_min} ((A[n][s][k] - e[n,s,k]) - last[s,k]) + seg_bonus
    W[n+1][k]  = max(W[n][k] + gap[n], X[n+1][k])
    path_score = max(G[N], max_k W[N][k])

NaN and -inf candidates are excluded, a NaN or +inf e excludes its cell.  Ties:
in A enter, stay, step, skip; in X the lowest s; in W the gap; in U the initial
term, then the lowest k'; at the end "no segment", then the lowest k.

``warpseg_reference`` is that loop, ``brute_force`` the enumeration of every
cover, label and move sequence it is checked against.  Along one path the loop
and the enumeration perform the same additions in the same order and rounding
is monotone, so their maxima are EQUAL, not merely close.

sp is the one place where the device's libm enters (exp and log1p in fp64, each
within 1 ulp).  ``warpseg_reference`` therefore takes cont / last as optional
arguments: the GPU tests read the two planes the kernel formed out of its state
tensor (``state_planes``), bound them against numpy's within SP_ULPS ulps, and
check the programme for EQUALITY on them.  exp and log1p within 1 ulp each and
one rounded addition give 2.5 ulps of the result at most; SP_ULPS = 4 leaves
room for numpy's own error."""
import functools
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import span_cases as SP  # noqa: E402
import syntax_cases as SY  # noqa: E402
import warp_cases as WC  # noqa: E402

NEG = SP.NEG
BAR = SP.BAR
MOVES = WC.MOVES
SP_ULPS = 4

PLANE_N = (1, 33, 70)
PLANE_K = (1, 33)
PLANE_T = (1, 5, 37)
PLANE_F = SP.ABI_F
PAD_LD = SP.PAD_LD

PROG_N = (1, 2, 33, 70)
PROG_KT = ((1, 1), (2, 3), (33, 37), (130, 5), (65, 20))
PROG_KINDS = ("random", "tied", "holes", "gaps", "zeros", "nopath")
PROG_SMIN = (0, 2)


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def softplus(v):
    return SP.softplus(np.asarray(v, dtype=np.float64))


def warpseg_reference(cost, v, log_move, log_enter, gap, seg_bonus, log_trans, log_init, s_min=0, cont=None,
                      last=None):
    """The recurrence above in a float64 loop over the frames.  cost is N x T x
    K (or N x T K), v is T x K.  -> dict(W (N + 1 x K), U (N x K), path_score,
    onset, length, cat, last_state, enter, exit, link (lists in time order))."""
    v = _f32(v)
    T, K = v.shape
    e_all = _f32(cost).reshape(-1, T, K)
    N = e_all.shape[0]
    lm = [float(m) for m in log_move]
    le = np.zeros(K) if log_enter is None else _f32(log_enter)
    lt, li = _f32(log_trans), _f32(log_init)
    g = None if gap is None else _f32(gap)
    bonus = np.float64(seg_bonus)
    cont = softplus(v) if cont is None else np.asarray(cont, dtype=np.float64).reshape(T, K)
    last = softplus(-v) if last is None else np.asarray(last, dtype=np.float64).reshape(T, K)
    cols = np.arange(K)
    G = 0.0
    W = np.full((N + 1, K), NEG)
    U = np.full((N, K), NEG)
    back_k = np.full((N, K), -1, dtype=np.int64)
    wsel = np.zeros((N + 1, K), dtype=np.int64)
    on = np.zeros((N + 1, K), dtype=np.int64)
    st = np.full((N + 1, K), -1, dtype=np.int64)
    X = np.full((N + 1, K), NEG)
    H = np.full((T, K), NEG)
    Hon = np.zeros((T, K), dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            c = W[n][:, None] + lt                    # (k', k)
            c = np.where(np.isnan(c), NEG, c)
            i = c.argmax(0)                           # the lowest k'
            best = c[i, cols]
            init = G + li
            vi, vp = init > NEG, best > NEG
            take_i = vi & (~vp | (init >= best))
            U[n] = np.where(take_i, init, np.where(vp, best, NEG))
            back_k[n] = np.where(take_i, -1, np.where(vp, i, -1))
            cand = np.full((4, T, K), NEG)
            ons = np.zeros((4, T, K), dtype=np.int64)
            cand[0, 0], ons[0, 0] = U[n] + le, n
            cand[1], ons[1] = H + lm[0], Hon
            if T > 1:
                cand[2, 1:], ons[2, 1:] = H[:-1] + lm[1], Hon[:-1]
            if T > 2:
                cand[3, 2:], ons[3, 2:] = H[:-2] + lm[2], Hon[:-2]
            cand = np.where(np.isnan(cand), NEG, cand)
            i = cand.argmax(0)                        # the first maximum: enter, stay, step, skip
            A = np.take_along_axis(cand, i[None], 0)[0]
            o = np.take_along_axis(ons, i[None], 0)[0]
            e = e_all[n]
            base = np.where(e < np.inf, A - e, NEG)   # False for NaN
            base = np.where(np.isnan(base), NEG, base)
            H, Hon = base - cont, o
            xc = base - last
            xc[:s_min] = NEG
            xc = np.where(np.isnan(xc), NEG, xc)
            si = xc.argmax(0)                         # the lowest s
            best = xc[si, cols]
            seg = best + bonus
            gv = g[n] if g is not None else NEG
            gapc = W[n] + gv
            vg, vs = gapc > NEG, (seg > NEG) & (best > NEG)
            take_g = vg & (~vs | (gapc >= seg))
            W[n + 1] = np.where(take_g, gapc, np.where(vs, seg, NEG))
            seg_won = ~take_g & vs
            wsel[n + 1] = seg_won
            on[n + 1] = o[si, cols]
            st[n + 1] = np.where(seg_won, si, -1)
            X[n + 1] = np.where(seg_won, seg, NEG)
            G = G + gv
    best, kb = (G if G > NEG else NEG), -1
    for k in range(K):
        if N and W[N, k] > best:
            best, kb = W[N, k], k
    keys = ("onset", "length", "cat", "last_state", "enter", "exit", "link")
    out = dict(W=W, U=U, path_score=float(best), **{key: [] for key in keys})
    n, k = N, kb
    while k >= 0 and n > 0:
        if not wsel[n, k]:
            n -= 1
            continue
        o = int(on[n, k])
        p = int(back_k[o, k])
        for key, val in zip(keys, (o, n - o, k, int(st[n, k]), float(U[o, k]), float(X[n, k]),
                                   float(li[k] if p < 0 else lt[p, k]))):
            out[key].append(val)
        n, k = o, p
    for key in keys:
        out[key].reverse()
    return out


def brute_force(cost, v, log_move, log_enter, gap, seg_bonus, log_trans, log_init, s_min=0):
    """Every cover by gap frames and segments, every label and every move
    sequence of a tiny case (N <= 5, K <= 2, T <= 3) -> (path_score, segments of
    the best cover as (onset, length, cat, last_state), how many covers attain
    it).  The additions of a path are the loop's, in its order."""
    v = _f32(v)
    T, K = v.shape
    e = _f32(cost).reshape(-1, T, K)
    N = e.shape[0]
    assert N <= 5 and K <= 2 and T <= 3
    lm = [float(m) for m in log_move]
    le = np.zeros(K) if log_enter is None else _f32(log_enter)
    lt, li = _f32(log_trans), _f32(log_init)
    g = None if gap is None else _f32(gap)
    bonus = np.float64(seg_bonus)
    cont, last = softplus(v), softplus(-v)
    found = []

    def alive(x):
        return x > NEG       # False for NaN

    def inside(n, k, s, a, onset, kp_value, segs):
        """frame n is emitted by state s of category k; a = A[n][s][k] along this path"""
        if not (e[n, s, k] < np.inf):
            return
        base = a - e[n, s, k]
        if not alive(base):
            return
        if s >= s_min:
            x = (base - last[s, k]) + bonus
            if alive(x):
                outside(n + 1, k, x, segs + [(onset, n + 1 - onset, k, s)])
        if n + 1 < N:
            h = base - cont[s, k]
            for m in range(3):
                if lm[m] > NEG and s + m < T and alive(h + lm[m]):
                    inside(n + 1, k, s + m, h + lm[m], onset, kp_value, segs)

    def outside(n, kp, value, segs):
        """before frame n; kp < 0: no segment yet and value = G[n], else value = W along this path"""
        if n == N:
            found.append((float(value), segs))
            return
        if g is not None and alive(value + g[n]):
            outside(n + 1, kp, value + g[n], segs)
        for k in range(K):
            u = value + (li[k] if kp < 0 else lt[kp, k])
            if alive(u) and alive(u + le[k]):
                inside(n, k, 0, u + le[k], n, None, segs)

    with np.errstate(invalid="ignore", over="ignore"):
        outside(0, -1, np.float64(0.0), [])
    if not found:
        return NEG, [], 0
    best = max(f[0] for f in found)
    winners = [f[1] for f in found if f[0] == best]
    return best, winners[0], len(winners)


def rigid_table(cost, v, s_min_unused=None):
    """The table abcd_span_table would hold for this plane with D = T and a zero
    weight, (N + 1) x T x K float64: entry [e, d - 1, k] = -(sum_{t < d} e[e - d +
    t, t, k]) - sum_{t < d - 1} sp(v[t, k]) - sp(-v[d - 1, k]), the frames in step
    order (span_cases.span_reference's order); -inf where d > e."""
    v = _f32(v)
    T, K = v.shape
    e = _f32(cost).reshape(-1, T, K)
    N = e.shape[0]
    O = SP.duration_reference(v, T)                       # K x T
    tab = np.full((N + 1, T, K), NEG)
    for end in range(1, N + 1):
        for d in range(1, min(T, end) + 1):
            E = np.zeros(K)
            for t in range(d):
                E = E + e[end - d + t, t]
            tab[end, d - 1] = 0.0 - E - O[:, d - 1]
    return tab


def log_softmax(x):
    return SY.log_softmax(x)


@functools.lru_cache(maxsize=None)
def prog_inputs(N, K, T, kind):
    """The inputs of one programme case on a GIVEN plane: dict(cost (N x T K
    fp32), v (T x K fp32), enter, gap, trans, init, bonus).  Shared, never
    modified.

    random  costs U[0, 6], logits N(0, 2), dense chain, drawn gap
    tied    small integers everywhere; the logits are +-800, where sp is 0 or
            800 exactly in any libm: every sum is exact and every tie occurs
    holes   the random plane with NaN and +inf entries and whole frames of them
    gaps    the random plane, a gap with -inf entries
    zeros   the chain with structural zeros, NaN entries, a dead row, a zero
            initial entry
    nopath  no gap and a plane whose frame N // 2 is all holes: no cover"""
    g = np.random.default_rng(15485863 * N + 7919 * K + 31 * T + PROG_KINDS.index(kind))
    S = K * T
    if kind == "tied":
        cost = g.integers(0, 3, size=(N, S)).astype(np.float32)
        v = np.where(g.random((T, K)) < 0.5, 800.0, -800.0).astype(np.float32)
        gap = g.integers(-3, 0, size=N).astype(np.float32)
        trans = g.integers(-2, 1, size=(K, K)).astype(np.float32)
        init = g.integers(-2, 1, size=K).astype(np.float32)
        enter = g.integers(-1, 1, size=K).astype(np.float32)
        bonus = -1.0
    else:
        cost = (g.random((N, S)) * 6.0).astype(np.float32)
        v = g.normal(0.0, 2.0, size=(T, K)).astype(np.float32)
        gap = g.normal(-4.0, 1.0, size=N).astype(np.float32)
        trans = np.stack([log_softmax(g.normal(0.0, 2.0, size=K)) for _ in range(K)]).astype(np.float32)
        init = log_softmax(g.normal(0.0, 1.0, size=K)).astype(np.float32)
        enter = g.normal(0.0, 1.0, size=K).astype(np.float32)
        bonus = 0.75
    if kind == "holes":
        cost[g.random(cost.shape) < 0.1] = np.nan
        cost[g.random(cost.shape) < 0.1] = np.inf
        for r in g.integers(0, N, size=max(N // 8, 1)):
            cost[r] = np.nan if r % 2 else np.inf
    if kind == "gaps":
        gap[g.random(N) < 0.2] = NEG
    if kind == "zeros":
        trans[g.random(trans.shape) < 0.3] = NEG
        trans[g.random(trans.shape) < 0.05] = np.nan
        trans[K // 2] = NEG
        init[K - 1] = NEG
    if kind == "nopath":
        cost[N // 2] = np.inf
        gap = None
    return dict(cost=cost, v=v, enter=enter, gap=gap, trans=trans, init=init, bonus=bonus)


def prog_reference(d, moves, s_min, cont=None, last=None):
    return warpseg_reference(d["cost"], d["v"], MOVES[moves], d["enter"], d["gap"], d["bonus"], d["trans"], d["init"],
                             s_min, cont, last)


def state_planes(state, N, K, T):
    """(cont, last), T x K float64 each, out of the state tensor (a numpy uint8 array) of warp_segment_window."""
    at = (N + 1) * K * 32
    S = K * T
    both = np.frombuffer(state[at:at + 16 * S].tobytes(), dtype=np.float64)
    return both[:S].reshape(T, K), both[S:].reshape(T, K)


def ulps_apart(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


# ----------------------------------------------------------------------------
# the emission plane
# ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plane_inputs(N, K, T, F):
    """x N(0, 1) around prototype rows, mu N(0, 1), lv U[-6, 2] (pairwise_cases' ranges), fp32.  Shared."""
    g = np.random.default_rng(1000003 * N + 10007 * K + 101 * T + F)
    mu = g.normal(size=(T * K, F)).astype(np.float32)
    lv = (g.random((T * K, F)) * 8.0 - 6.0).astype(np.float32)
    rows = g.integers(0, T * K, size=N)
    x = (mu[rows] + g.normal(size=(N, F)) * np.exp(0.5 * lv[rows]) * 1.5).astype(np.float32)
    return dict(x=x, mu=mu, lv=lv)


@functools.lru_cache(maxsize=None)
def plane_reference(N, K, T, F):
    """(e, unit), N x T K float64: the emission term and score_cases' unit, 0.5 sum_f (log 2pi + |lv| + d^2 e^-lv)."""
    d = plane_inputs(N, K, T, F)
    x, mu, lv = (np.asarray(d[k], dtype=np.float64) for k in ("x", "mu", "lv"))
    e, unit = np.zeros((N, T * K)), np.zeros((N, T * K))
    for n in range(N):
        q = (x[n][None] - mu) ** 2 * np.exp(-lv)
        e[n] = (0.5 * (WC.LOG2PI + lv + q)).sum(-1)
        unit[n] = (0.5 * (WC.LOG2PI + np.abs(lv) + q)).sum(-1)
    return e, unit


# ----------------------------------------------------------------------------
# the planted recording: a tempo the rigid template cannot follow
# ----------------------------------------------------------------------------
PLANT_K, PLANT_S, PLANT_F = 4, 12, 9
# (category, the states its frames are decoded at): slow (stays), fast (skips), mixed, and one at the prototype's tempo
PLANT_SEGMENTS = ((2, [t // 2 for t in range(24)]),
                  (0, [min(2 * t, 11) for t in range(6)] + [11]),
                  (3, [0, 0, 1, 2, 4, 6, 7, 7, 7, 8, 10, 11]),
                  (1, list(range(12))),
                  (2, [0, 1, 1, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 9, 10, 11, 11]))
PLANT_MOVES = MOVES["default"]


@functools.lru_cache(maxsize=None)
def planted():
    """A recording concatenated from prototypes decoded along warp_cases.PLANTS-
    style state paths plus 0.05 N(0, 1): mu N(0, 1), lv = -2, offset logits -8
    except +8 at the last state.  dict(x, mu, lv (T K x F), v (T x K), onset,
    length, cat, trans, init (uniform), N)."""
    g = np.random.default_rng(271828)
    T, K, F = PLANT_S, PLANT_K, PLANT_F
    mu = g.normal(size=(T, K, F)).astype(np.float32)
    lv = np.full((T, K, F), -2.0, dtype=np.float32)
    v = np.full((T, K), -8.0, dtype=np.float32)
    v[T - 1] = 8.0
    xs, onset, length, cat = [], [], [], []
    at = 0
    for k, path in PLANT_SEGMENTS:
        xs.append(mu[np.array(path), k] + 0.05 * g.normal(size=(len(path), F)).astype(np.float32))
        onset.append(at)
        length.append(len(path))
        cat.append(k)
        at += len(path)
    x = np.concatenate(xs).astype(np.float32)
    trans = np.full((K, K), math.log(1.0 / K), dtype=np.float32)
    init = np.full(K, math.log(1.0 / K), dtype=np.float32)
    return dict(x=x, mu=mu.reshape(T * K, F), lv=lv.reshape(T * K, F), v=v, onset=onset, length=length, cat=cat,
                trans=trans, init=init, N=at, K=K, T=T, F=F)


@functools.lru_cache(maxsize=None)
def planted_plane():
    """e (N x T K float64) of the planted recording, in float64."""
    d = planted()
    x, mu, lv = (np.asarray(d[k], dtype=np.float64) for k in ("x", "mu", "lv"))
    return np.stack([(0.5 * (WC.LOG2PI + lv + (x[n][None] - mu) ** 2 * np.exp(-lv))).sum(-1) for n in range(d["N"])])


def planted_references():
    """(warped, rigid): warpseg_reference under PLANT_MOVES and syntax_cases.chain_reference on the rigid table
    of the same plane, both without a gap: every frame belongs to a segment."""
    d = planted()
    e = planted_plane()
    warped = warpseg_reference(e, d["v"], PLANT_MOVES, None, None, 0.0, d["trans"], d["init"], 0)
    rigid = SY.chain_reference(rigid_table(e, d["v"]), 1, d["trans"], d["init"], None, 0.0)
    return warped, rigid


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as span_cases.dump)."""
    SP.PW.E.dump_observed("warpseg_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/warpseg_errors.json from a run of tests/test_gpu_warpseg.py with ABCD_PARITY_DUMP=<dump_dir>."""
    import glob
    import json
    rows = {}
    for kind in ("plane", "prog", "e2e"):
        rows[kind] = []
        for path in sorted(glob.glob(os.path.join(dump_dir, f"warpseg_{kind}_*.json"))):
            with open(path) as f:
                rows[kind] += json.load(f)
    worst = dict(plane=max((r["plane"] for r in rows["plane"]), default=None),
                 sp_ulps=max((r["sp_ulps"] for r in rows["prog"]), default=None),
                 e2e_score=max((r["score"] for r in rows["e2e"] if "score" in r), default=None))
    doc = dict(what="figures observed by tests/test_gpu_warpseg.py (ABCD_PARITY_DUMP) on one MI355X; units and bars: "
                    "tests/warpseg_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(plane=BAR, sp_ulps=SP_ULPS, programme="equality", windows="bit equality", e2e_score=WC.BAR),
               worst=worst, **rows)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/warpseg_cases.py <dump directory> <out.json> <date> <parent commit>
    print(assemble(*sys.argv[1:5])["worst"])
