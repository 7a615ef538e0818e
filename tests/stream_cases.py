"""Cases and the float64 reference of syntax-aware segmentation with the table
in windows (``abcd_span_chain_viterbi_window``, ``segmentation.plan_windows``,
``segment_frames(..., window_frames=W)``).  ``syntax_cases`` is
imported and left as it is: its ``chain_reference`` on the whole table is what
every windowed result must equal bit for bit, and its ``chain_inputs`` are the
inputs.

``windowed_reference`` runs ``chain_reference``'s recurrences window by window:
each window sees only its own slice of the table (rows ``row0 .. n1``, the rows
below ``n0 - row0`` NaN), and what crosses from one window to the next is what
the kernel carries: the lattice ``U``, the two back-pointer planes, the chosen
entries ``sel``, and the carry ``(W[n1], G[n1], next_n)``."""
import functools

import numpy as np
import torch

import syntax_cases as SX

NEG = SX.NEG
ALIGN = 32                       # the table pass's start tile

STREAM_ND = SX.CHAIN_ND          # (1, 1), (2, 1), (33, 5), (33, 37), (70, 17)
STREAM_K = SX.CHAIN_K            # 1, 2, 33, 65, 130 (130 streams log_trans)
WIDTH_K = (256, 257)             # the launch-width threshold, at (33, 5)
REF_ND = ((33, 5), (33, 37), (70, 17))
PLAN_N = (1, 2, 33, 133, 15000)
PLAN_D = (1, 5, 17, 37, 200)
LONG_ND = (150000, 200)          # beyond the one-shot limit at K = 128
SLICE_N, SLICE_D, SLICE_P, SLICE_F = 133, (17, 37), (1, 33), 65
SLICE_W = (40, 16)


def window_sizes(N, D):
    """W in 1, 3, D, N, without repeats, in that order."""
    out = []
    for w in (1, 3, D, N):
        if w not in out:
            out.append(w)
    return out


def plan(N, D, W, align=ALIGN):
    """The windows as the issue defines them, written independently of
    ``segmentation.plan_windows``: [(row0, n0, n1)]."""
    out = []
    for n0 in range(1, N + 1, W):
        out.append((align * (max(0, n0 - D) // align), n0, min(N, n0 + W - 1)))
    return out


def window_of(table, row0, n0, n1):
    """Rows row0 .. n1 of the whole table as an array of its own; the rows below
    n0 - row0 (which the programme must not read) hold NaN."""
    w = np.array(table[row0:n1 + 1], dtype=np.float64, copy=True)
    w[:n0 - row0] = np.nan
    return w


def new_state(N, K):
    """What is carried, before the first window: everything poisoned."""
    return dict(U=np.full((N + 1, K), np.nan), back_d=np.full((N + 1, K), -99, dtype=np.int64),
                back_k=np.full((N + 1, K), -99, dtype=np.int64), sel=np.full((N + 1, K), np.nan),
                W=np.full((N + 1, K), np.nan), Wc=np.full(K, np.nan), G=np.nan, next_n=-1)


def window_step(st, Twin, row0, n0, n1, N, d_min, log_trans, log_init, gap, seg_bonus):
    """Steps n0 .. n1 of ``syntax_cases.chain_reference`` on the window ``Twin``
    (row 0 = end row0), every statement of its loop with ``T[n]`` replaced by
    ``Twin[n - row0]``.  Returns False (and does nothing) when the call is out
    of order."""
    D, K = Twin.shape[1], Twin.shape[2]
    lt, li = SX._f32(log_trans), SX._f32(log_init)
    g = None if gap is None else SX._f32(gap)
    bonus = np.float64(seg_bonus)
    if n0 == 1:
        st["U"][0] = li
        st["back_k"][0] = -1
        st["W"][0] = NEG
        st["Wc"] = np.full(K, NEG)
        st["G"] = np.float64(0.0)
    elif st["next_n"] != n0:
        return False
    U, W, back_d, back_k, sel = st["U"], st["W"], st["back_d"], st["back_k"], st["sel"]
    Wc, G = st["Wc"], st["G"]
    cols = np.arange(K)
    with np.errstate(invalid="ignore"):
        for n in range(n0, n1 + 1):
            Trow = Twin[n - row0]
            G = G + (g[n - 1] if g is not None else NEG)
            hi = min(D, n)
            best = np.full(K, NEG)
            bd = np.zeros(K, dtype=np.int64)
            if hi >= d_min:
                c = U[n - d_min:(n - hi - 1 if n > hi else None):-1] + Trow[d_min - 1:hi]     # (d, k)
                c = np.where(np.isnan(c), NEG, c)
                i = c.argmax(0)
                best, bd = c[i, cols], d_min + i
            seg = best + bonus
            gapc = Wc + g[n - 1] if g is not None else np.full(K, NEG)
            vg, vs = gapc > NEG, (seg > NEG) & (best > NEG)
            take_g = vg & (~vs | (gapc >= seg))
            Wc = np.where(take_g, gapc, np.where(vs, seg, NEG))
            W[n] = Wc
            back_d[n] = np.where(take_g, 0, np.where(vs, bd, 0))
            sel[n] = np.where(back_d[n] > 0, Trow[np.maximum(back_d[n], 1) - 1, cols], NEG)
            if n == N:
                break
            c = Wc[:, None] + lt
            c = np.where(np.isnan(c), NEG, c)
            i = c.argmax(0)
            best = c[i, cols]
            init = G + li
            vi, vp = init > NEG, best > NEG
            take_i = vi & (~vp | (init >= best))
            U[n] = np.where(take_i, init, np.where(vp, best, NEG))
            back_k[n] = np.where(take_i, -1, np.where(vp, i, -1))
    st["Wc"], st["G"], st["next_n"] = Wc, G, n1 + 1
    return True


def finish(st, N, log_trans, log_init):
    """The end of ``chain_reference`` on the carried state: path_score and the
    backtrack, the segment's score from ``sel``."""
    lt, li = SX._f32(log_trans), SX._f32(log_init)
    K = st["Wc"].shape[0]
    best, kb = (st["G"] if st["G"] > NEG else NEG), -1
    for k in range(K):
        if st["Wc"][k] > best:
            best, kb = st["Wc"][k], k
    out = dict(W=st["W"], path_score=float(best), onset=[], length=[], cat=[], score=[], link=[])
    n, k = N, kb
    while k >= 0 and n > 0:
        d = int(st["back_d"][n, k])
        if d == 0:
            n -= 1
            continue
        out["onset"].append(n - d)
        out["length"].append(d)
        out["cat"].append(k)
        out["score"].append(float(st["sel"][n, k]))
        n -= d
        p = int(st["back_k"][n, k])
        out["link"].append(float(li[k] if p < 0 else lt[p, k]))
        k = p
    for key in ("onset", "length", "cat", "score", "link"):
        out[key].reverse()
    return out


def windowed_reference(table, d_min, log_trans, log_init, gap, seg_bonus, windows):
    """``chain_reference``'s dict from the windows ``[(row0, n0, n1)]`` in order."""
    T = np.asarray(table, dtype=np.float64)
    N, K = T.shape[0] - 1, T.shape[2]
    st = new_state(N, K)
    for row0, n0, n1 in windows:
        assert window_step(st, window_of(T, row0, n0, n1), row0, n0, n1, N, d_min, log_trans, log_init, gap, seg_bonus)
    return finish(st, N, log_trans, log_init)


@functools.lru_cache(maxsize=None)
def reference(N, D, K, kind, call, init_key="init"):
    """``chain_reference`` of call number ``call`` of ``chain_inputs(N, D, K,
    kind)``, computed once and shared."""
    c = SX.chain_inputs(N, D, K, kind)
    d_min, gap, bonus, _ = c["calls"][call]
    return SX.chain_reference(c["table"], d_min, c["trans"], c[init_key], gap, bonus)


def same_result(a, b):
    """Two ``chain_reference``-shaped dicts agree bit for bit."""
    if not np.array_equal(np.asarray(a["W"]).view(np.int64), np.asarray(b["W"]).view(np.int64)):
        return False
    if np.float64(a["path_score"]).view(np.int64) != np.float64(b["path_score"]).view(np.int64):
        return False
    for key in ("onset", "length", "cat"):
        if list(a[key]) != list(b[key]):
            return False
    for key in ("score", "link"):
        x, y = np.asarray(a[key], dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        if x.shape != y.shape or not np.array_equal(x.view(np.int64), y.view(np.int64)):
            return False
    return True


@functools.lru_cache(maxsize=None)
def slice_inputs(N, D, P, F):
    """Random fp32 inputs of the table pass drawn as ``span_cases.abi_inputs``
    draws them, without its float64 reference (the slices are compared with the
    one-shot table, not with a reference).  Shared, never modified."""
    g = torch.Generator().manual_seed(7919 * N + 10007 * D + 101 * P + F)
    T = D + SX.SP.T_EXTRA
    mu = torch.randn(T, P, F, generator=g)
    lv = torch.rand(T, P, F, generator=g) * 8.0 - 6.0
    o = torch.rand(T, P, generator=g) * 16.0 - 8.0
    lw = torch.randn(P, generator=g)
    x = torch.empty(N, F)
    at = 0
    while at < N:
        d = min(int(torch.randint(1, D + 1, (1,), generator=g)), N - at)
        p = int(torch.randint(0, P, (1,), generator=g))
        x[at:at + d] = mu[:d, p] + torch.randn(d, F, generator=g) * torch.exp(0.5 * lv[:d, p]) * 1.5
        at += d
    return dict(N=N, D=D, P=P, F=F, T=T, x=x, mu=mu, lv=lv, o=o, lw=lw)
