"""Cases and the float64 oracle of the category-sequence HMM
(``abcd_chain_posterior``, ``torch.ops.abcd.chain_posterior``,
``modules.sequence.TransitionModel``, ``sequence.py``).

The oracle is a plain log-domain forward-backward, Viterbi and expected counts
in numpy on the SAME fp32 inputs, nothing renormalised:

    alpha_0 = log_init + score_0
    alpha_t+1[j] = score_t+1[j] + logsumexp_i(alpha_t[i] + log_trans[i, j])
    log_evidence = logsumexp_k alpha_T-1[k]
    beta_T-1 = 0,  beta_t[i] = logsumexp_j(log_trans[i, j] + score_t+1[j] + beta_t+1[j])
    gamma_t = exp(alpha_t + beta_t - log_evidence)
    xi_t[i, j] = exp(alpha_t[i] + log_trans[i, j] + score_t+1[j] + beta_t+1[j] - log_evidence)

with the exclusion rules of the header: a NaN or +inf score counts as -inf; a
sequence without forward mass gets log_evidence = -inf, gamma = 0, path = -1,
path_score = -inf and no counts; a zero-length sequence gets log_evidence = 0
and nothing else (its path_score entry stays NaN here).  ``dtype=np.float32``
runs the same code in float32: its distance from the float64 run is the ``e32``
the GPU bars are made of.
"""
import functools
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import edge_cases as E  # noqa: E402

ORDER_FACTOR = 4.0               # the project's allowance for a different summation order (vocoder_cases.py)
CAST_FLOOR = 2.0 ** -22          # the final cast, with the factor of 4 (pairwise_cases.LOGEV_BAR)
DECIDED_GAP = 0.05               # nats by which every back-pointer of a decided path wins in float64
UNDECIDED_CAP = 0.1              # at most one generated sequence in ten may fall outside "decided"
LENGTHS = (0, 1, 2, 3, 17, 300)
PAD = 3                          # NaN columns after the K real ones
WANT_EVIDENCE, WANT_GAMMA, WANT_PATH, WANT_COUNTS = 1, 2, 4, 8


# ----------------------------------------------------------------------------
# the oracle
# ----------------------------------------------------------------------------
def _clean(x, dtype):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        ok = (x > -np.inf) & (x < np.inf)
    return np.where(ok, x, -np.inf).astype(dtype)


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    mm = np.where(m > -np.inf, m, 0).astype(x.dtype)
    with np.errstate(divide="ignore"):
        out = mm + np.log(np.exp(x - mm).sum(axis=axis, keepdims=True, dtype=x.dtype))
    return np.squeeze(out, axis=axis)


def _gap(v):
    """the best entry minus the second best (inf with one entry)"""
    if v.shape[0] == 1:
        return np.inf
    top = np.partition(v, -2)[-2:]
    with np.errstate(invalid="ignore"):
        g = top[1] - top[0]
    return np.inf if np.isnan(g) else float(g)


def oracle(score, seq_off, log_trans, log_init, dtype=np.float64):
    """dict(log_evidence S, gamma N x K, path N, path_score S, trans_counts K x
    K, init_counts K, decided S bool, counts_by_length {T: K x K}): see the
    module docstring.  score / log_trans may carry padding columns (only the
    first K are read, K = len(log_init))."""
    li = _clean(log_init, dtype)
    K = li.shape[0]
    lt = _clean(np.asarray(log_trans)[:K, :K], dtype)
    sc = _clean(np.asarray(score)[:, :K], dtype)
    off = np.asarray(seq_off, dtype=np.int64)
    S, N = len(off) - 1, sc.shape[0]
    ev = np.zeros(S, dtype=dtype)
    gamma = np.zeros((N, K), dtype=dtype)
    path = np.full(N, -1, dtype=np.int64)
    ps = np.full(S, np.nan, dtype=dtype)
    tc, ic = np.zeros((K, K), dtype=dtype), np.zeros(K, dtype=dtype)
    decided = np.ones(S, dtype=bool)
    by_len = {}
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(S):
            r0, T = int(off[s]), int(off[s + 1] - off[s])
            if T == 0:
                continue
            x = sc[r0:r0 + T]
            alpha = np.empty((T, K), dtype=dtype)
            alpha[0] = li + x[0]
            for t in range(1, T):
                alpha[t] = x[t] + _lse(alpha[t - 1][:, None] + lt, 0)
            z = _lse(alpha[-1], 0)
            if not z > -np.inf:
                ev[s], ps[s] = -np.inf, -np.inf
                continue
            ev[s] = z
            beta = np.zeros((T, K), dtype=dtype)
            cnt = np.zeros((K, K), dtype=dtype)
            for t in range(T - 2, -1, -1):
                w = x[t + 1] + beta[t + 1]
                beta[t] = _lse(lt + w[None, :], 1)
                cnt += np.exp(alpha[t][:, None] + lt + w[None, :] - z)
            gamma[r0:r0 + T] = np.exp(alpha + beta - z)
            tc += cnt
            ic += gamma[r0]
            by_len[T] = by_len.get(T, 0) + cnt
            # Viterbi: argmax is the lowest index of the maximum
            delta = li + x[0]
            bp = np.zeros((T, K), dtype=np.int64)
            cand = []
            for t in range(1, T):
                c = delta[:, None] + lt
                bp[t] = c.argmax(0)
                cand.append(c)
                delta = x[t] + c.max(0)
            p = int(delta.argmax())
            ps[s] = delta[p]
            ok = _gap(delta) >= DECIDED_GAP
            for t in range(T - 1, 0, -1):
                path[r0 + t] = p
                ok = ok and _gap(cand[t - 1][:, p]) >= DECIDED_GAP
                p = int(bp[t][p])
            path[r0] = p
            decided[s] = ok
    return dict(log_evidence=ev, gamma=gamma, path=path, path_score=ps, trans_counts=tc, init_counts=ic,
                decided=decided, counts_by_length=by_len)


def path_log_joint(path, score, seq_off, log_trans, log_init):
    """The float64 log joint of a given state path, per sequence (-inf for a
    path of -1, nan for a zero-length sequence)."""
    li = _clean(log_init, np.float64)
    K = li.shape[0]
    lt = _clean(np.asarray(log_trans)[:K, :K], np.float64)
    sc = _clean(np.asarray(score)[:, :K], np.float64)
    off = np.asarray(seq_off, dtype=np.int64)
    out = np.full(len(off) - 1, np.nan)
    for s in range(len(off) - 1):
        p = np.asarray(path[off[s]:off[s + 1]], dtype=np.int64)
        if len(p) == 0:
            continue
        if (p < 0).any():
            out[s] = -np.inf
            continue
        rows = np.arange(off[s], off[s + 1])
        out[s] = li[p[0]] + sc[rows, p].sum() + lt[p[:-1], p[1:]].sum()
    return out


def brute_force(score, log_trans, log_init):
    """One sequence by enumeration of all K^T paths (float64): dict(log_evidence,
    gamma, trans_counts, init_counts, path, path_score); the best path is the
    one Viterbi's lowest-index rule returns: ties are broken at the LAST step
    first (the final state, then each back-pointer in turn)."""
    import itertools
    sc, lt, li = (np.asarray(v, dtype=np.float64) for v in (score, log_trans, log_init))
    T, K = sc.shape
    paths = list(itertools.product(range(K), repeat=T))
    lj = np.array([li[p[0]] + sum(sc[t, p[t]] for t in range(T)) + sum(lt[p[t], p[t + 1]] for t in range(T - 1))
                   for p in paths])
    m = lj.max()
    z = m + np.log(np.exp(lj - m).sum())
    w = np.exp(lj - z)
    gamma, tc = np.zeros((T, K)), np.zeros((K, K))
    for p, wi in zip(paths, w):
        for t in range(T):
            gamma[t, p[t]] += wi
        for t in range(T - 1):
            tc[p[t], p[t + 1]] += wi
    best = [p for p, v in zip(paths, lj) if v == m]
    best.sort(key=lambda p: p[::-1])
    return dict(log_evidence=z, gamma=gamma, trans_counts=tc, init_counts=gamma[0].copy(),
                path=np.array(best[0]), path_score=m)


# ----------------------------------------------------------------------------
# generated cases
# ----------------------------------------------------------------------------
def plan(K, S):
    """(resident, workgroups) from abcd_chain_plan (a pure host function)."""
    import ctypes
    from modules import _native as N
    res, wg = ctypes.c_int(0), ctypes.c_int(0)
    assert N.lib().abcd_chain_plan(int(K), int(S), res, wg) == 0
    return bool(res.value), int(wg.value)


@functools.lru_cache(maxsize=None)
def first_streaming_k():
    """the first K abcd_chain_plan calls non-resident"""
    return next(K for K in range(1, 1025) if not plan(K, 1)[0])


def case_ks():
    return (1, 5, 64, 65, 128, first_streaming_k(), 1024)


S_KINDS = ("one", "three", "many")


def case_ids():
    return [(K, kind) for K in case_ks() for kind in S_KINDS]


def _lengths(K, kind, g):
    """Lengths from LENGTHS; K = 1024 stays within N <= 64."""
    small = K >= 1024
    if kind == "one":
        return [17 if small else 300]
    if kind == "three":
        return [17, 0, 3] if small else [17, 0, 300]
    S = 2 * plan(K, 1 << 20)[1] + 1          # every workgroup takes several sequences
    if small:                                # mostly empty sequences: 7 each of lengths 1, 2, 3 and one of 17
        lens = [0] * S
        for n, s in enumerate(g.choice(S, size=21, replace=False)):
            lens[s] = 1 + n % 3
        lens[1] = 17
        return lens
    lens = g.choice([0, 1, 2, 3], size=S).tolist()
    lens[1] = 17
    lens[S // 2] = 300
    return lens


def draw_chain(K, g, zeros=True):
    """(trans K x K, init K) float64 probabilities: sparse Dirichlet(0.1) rows,
    a tenth of the entries then set to exactly zero (never a row's largest)."""
    trans = g.dirichlet(np.full(K, 0.1), size=K)
    if zeros and K > 1:
        kill = g.random((K, K)) < 0.1
        kill[np.arange(K), trans.argmax(1)] = False
        trans = np.where(kill, 0.0, trans)
    trans = trans / trans.sum(1, keepdims=True)
    init = g.dirichlet(np.full(K, 0.5))
    init = np.maximum(init, 1e-300)
    return trans, init / init.sum()


def draw_scores(z, K, g):
    """Row-normalised scores around the state sequence z: the true state at 0,
    two runners-up 2 to 6 nats behind, in a fifth of the rows one more state
    within 0.5 of the leader, the rest 20 to 200 behind."""
    n = len(z)
    sc = -(20.0 + 180.0 * g.random((n, K)))
    for r in range(n):
        others = [k for k in g.permutation(K) if k != z[r]][:3]
        for k in others[:2]:
            sc[r, k] = -(2.0 + 4.0 * g.random())
        if len(others) > 2 and g.random() < 0.2:
            sc[r, others[2]] = -0.5 * g.random()
        sc[r, z[r]] = 0.0
    return sc


@functools.lru_cache(maxsize=None)
def case(K, kind):
    """One generated corpus: dict(K, seq_off, score (N x K + PAD, NaN padding),
    log_trans (K x K + PAD, NaN padding), log_init, ref (float64 oracle), ref32
    (float32 oracle)), fp32 inputs as torch tensors.  Shared, never modified."""
    import torch
    g = np.random.default_rng(7919 * K + S_KINDS.index(kind))
    lens = _lengths(K, kind, g)
    trans, init = draw_chain(K, g)
    z = []
    for T in lens:                       # the true states follow the chain: every sequence has a path
        for t in range(T):
            p = init if t == 0 else trans[z[-1]]
            z.append(int(g.choice(K, p=p)))
    sc = draw_scores(z, K, g)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with np.errstate(divide="ignore"):
        lt, li = np.log(trans).astype(np.float32), np.log(init).astype(np.float32)
    score = np.full((len(z), K + PAD), np.nan, dtype=np.float32)
    score[:, :K] = sc.astype(np.float32)
    ltp = np.full((K, K + PAD), np.nan, dtype=np.float32)
    ltp[:, :K] = lt
    ref = oracle(score, seq_off, ltp, li)
    ref32 = oracle(score, seq_off, ltp, li, dtype=np.float32)
    return dict(K=K, kind=kind, lengths=lens, seq_off=torch.from_numpy(seq_off), score=torch.from_numpy(score),
                log_trans=torch.from_numpy(ltp), log_init=torch.from_numpy(li), ref=ref, ref32=ref32)


def rel_err(got, ref):
    """max |got - ref| / |ref| over the finite entries of ref (0 / 0 counts as 0);
    entries where ref is not finite must agree exactly (NaN with NaN)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    fin = np.isfinite(ref)
    same = (got[~fin] == ref[~fin]) | (np.isnan(got[~fin]) & np.isnan(ref[~fin]))
    assert same.all(), (got[~fin], ref[~fin])
    d, a = np.abs(got[fin] - ref[fin]), np.abs(ref[fin])
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(d == 0, 0.0, d / a)
    return float(r.max()) if r.size else 0.0


def bars(c):
    """The bars of one case, from the float32 oracle's own error (e32) on the
    same inputs: dict(evidence, path_score: relative, max(2^-22, 4 e32); gamma,
    counts: absolute, 4 e32) and the e32 figures themselves."""
    r, r32 = c["ref"], c["ref32"]
    e = dict(evidence=rel_err(r32["log_evidence"], r["log_evidence"]),
             path_score=rel_err(r32["path_score"], r["path_score"]),
             gamma=float(np.abs(r32["gamma"] - r["gamma"]).max()) if r["gamma"].size else 0.0,
             counts=max(float(np.abs(r32["trans_counts"] - r["trans_counts"]).max()),
                        float(np.abs(r32["init_counts"] - r["init_counts"]).max())))
    return dict(e32=e, evidence=max(CAST_FLOOR, ORDER_FACTOR * e["evidence"]),
                path_score=max(CAST_FLOOR, ORDER_FACTOR * e["path_score"]), gamma=ORDER_FACTOR * e["gamma"],
                counts=ORDER_FACTOR * e["counts"])


def em_reference(score, seq_off, log_trans, log_init, n_iter, pseudo_count):
    """The oracle's EM in float64: the objective before the first iteration and
    after each one (n_iter + 1 values), M-step (counts + c) normalised; the
    parameters pass through float32 after every M-step as the model's buffers
    do."""
    lt, li = np.asarray(log_trans, dtype=np.float64), np.asarray(log_init, dtype=np.float64)
    K = li.shape[0]
    lt = lt[:K, :K]
    c = float(pseudo_count)

    def objective(ev):
        return ev.sum() + c * (lt[np.isfinite(lt)].sum() + li[np.isfinite(li)].sum())
    objs = []
    for _ in range(n_iter):
        r = oracle(score, seq_off, lt, li)
        objs.append(objective(r["log_evidence"]))
        t, i = r["trans_counts"] + c, r["init_counts"] + c
        with np.errstate(divide="ignore"):
            lt = np.log(t / t.sum(1, keepdims=True)).astype(np.float32).astype(np.float64)
            li = np.log(i / i.sum()).astype(np.float32).astype(np.float64)
    objs.append(objective(oracle(score, seq_off, lt, li)["log_evidence"]))
    return np.array(objs)


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    E.dump_observed("chain_" + name, rows)


def collect(src):
    """Assemble profiles/chain_errors.json from the files a GPU run of
    tests/test_gpu_chain.py left in ``src`` (``ABCD_PARITY_DUMP=<src>``)."""
    import glob
    import json
    rows = []
    for path in glob.glob(os.path.join(src, "chain_k*.json")):
        with open(path) as f:
            rows.append(json.load(f))
    rows.sort(key=lambda r: (r["K"], S_KINDS.index(r["kind"])))
    with open(os.path.join(src, "chain_pair_posterior.json")) as f:
        pair = json.load(f)
    doc = dict(note="figures observed by tests/test_gpu_chain.py on an MI355X (ABCD_PARITY_DUMP): errors against the "
                    "float64 oracle of tests/chain_cases.py beside their bars (4 x the float32 oracle's own error e32; "
                    "evidence and path_score relative with a floor of 2^-22, gamma and counts absolute)",
               cases=rows, pair_posterior=pair)
    out = os.path.join(REPO, "profiles", "chain_errors.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return out


if __name__ == "__main__":  # python tests/chain_cases.py <dump directory>
    print(collect(sys.argv[1]))
