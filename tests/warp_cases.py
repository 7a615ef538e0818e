"""Cases and the float64 references of time-warped scoring (``abcd_warp_nll``,
``abcd_warp_path``, ``RNN_Variational_Decoder.warp_against`` / ``align_to``,
``modules/alignment.py``, ``align.py``): DESIGN.md s3.11 in its written form.

The prototype's steps are the states of a left-to-right HMM.  Frame t of a
segment is emitted by state a(t), a(0) = 0, a(t + 1) - a(t) in {0, 1, 2} (stay,
step, skip) at a cost of -log_move[m]; cells with |s - t| > band do not exist
(band < 0: no band).  With r = off_t + b,

    e(t,s) = 0.5 sum_f (log 2pi + lv[s,p,f] + (x[r,f] - mu[s,p,f])^2 e^-lv[s,p,f])
    o(t,s) = max(v,0) - v y[r] + log1p(e^-|v|),  v = logits[s, p]
    c(t,s) = e(t,s) + o(t,s)
    D[0,0] = c(0,0);  D[0,s>0] = +inf
    D[t,s] = c(t,s) + (+)_{m, s-m >= 0} (D[t-1,s-m] - log_move[m])
    warp[b,p] = (+)_s D[len_b - 1, s]

with (+) = min (Viterbi) or -log sum exp(-.) (marginal).  A disabled move
(-inf), a +inf predecessor, a cell outside the band and a NaN cost are
excluded; a cell with nothing left is +inf.  Viterbi ties go to the lowest
move, then to the lowest final state.

``dp`` is that recurrence on a given cost plane, ``brute_force`` the
enumeration of every move sequence it is checked against, ``warp_reference``
the whole thing on the fp32 inputs the kernels read.  Errors are measured in
the unit ``A[b,p]``: along the float64 Viterbi path, the sum of the emission
unit of ``score_cases`` (0.5 sum_f (log 2pi + |lv| + d^2 e^-lv)) of every
visited cell, of its |o| and of the |log_move| of every move taken.
``pairwise_cases`` and ``score_cases`` are imported and left as they are.
"""
import functools
import itertools
import math
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import edge_cases as E  # noqa: E402
import pairwise_cases as PW  # noqa: E402
import score_cases as S  # noqa: E402

LOG2PI = S.LOG2PI
BAR = S.BAR                      # 1e-4 of the unit, the project's loss bar
cross_bar = PW.cross_bar
NINF = -math.inf
MOVES = dict(default=(math.log(0.2), math.log(0.6), math.log(0.2)),
             identity=(NINF, 0.0, NINF),
             staystep=(math.log(0.5), math.log(0.5), NINF),
             stepskip=(NINF, math.log(0.5), math.log(0.5)))
# the shapes of pairwise_cases the ABI cases use, and one more: the recurrence walks the states in super-blocks
# of 128, which none of those shapes reaches (37 frames reach 73 states); 170 frames reach 339, three super-blocks,
# and under a band the lower super-blocks are left behind as the frames advance
ABI_SHAPES = OrderedDict((k, PW.ABI_SHAPES[k]) for k in ("b1t1", "ties", "b33t9", "b40t37"))
ABI_SHAPES["b3t170"] = [170, 131, 40]
PAD_LD = PW.PAD_LD


# ----------------------------------------------------------------------------
# the recurrence and its brute-force check
# ----------------------------------------------------------------------------
def _exists(S_, t, band):
    s = np.arange(S_)
    return np.ones(S_, dtype=bool) if band < 0 else np.abs(s - t) <= band


def dp(c, lens, log_move, band=-1, marginal=False):
    """The recurrence on cost planes c (... x T x S, NaN = excluded) for
    segments of lens (...) frames -> dict(value (...), back (... x T x S, the
    move into each cell, Viterbi only), end (...): the final state, -1 if none)."""
    c = np.asarray(c, dtype=np.float64)
    lead, (T, S_) = c.shape[:-2], c.shape[-2:]
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int64), lead)
    lm = [float(v) for v in log_move]
    cc = np.where(np.isnan(c), np.inf, c)
    D = np.full(lead + (S_,), np.inf)
    D[..., 0] = cc[..., 0, 0]
    back = np.full(lead + (T, S_), -1, dtype=np.int8)
    final = np.where((lens == 1)[..., None], D, np.inf)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for t in range(1, T):
            cand = np.full((3,) + lead + (S_,), np.inf)
            for m in range(3):
                if lm[m] > NINF and S_ > m:
                    cand[m][..., m:] = D[..., :S_ - m] - lm[m]
            mn = cand.min(0)
            if marginal:
                some = mn < np.inf
                ex = np.exp(np.where(cand < np.inf, np.where(some, mn, 0.0)[None] - cand, NINF))
                tot = np.where(some, mn - np.log(np.where(some, ex.sum(0), 1.0)), np.inf)
            else:
                tot = mn
                back[..., t, :] = np.where(mn < np.inf, cand.argmin(0), -1)   # argmin: the lowest move of the minimum
            D = np.where(_exists(S_, t, band), cc[..., t, :] + tot, np.inf)
            final = np.where((lens == t + 1)[..., None], D, final)
        mn = final.min(-1)
        some = mn < np.inf
        if marginal:
            ex = np.exp(np.where(final < np.inf, np.where(some, mn, 0.0)[..., None] - final, NINF))
            value = np.where(some, mn - np.log(np.where(some, ex.sum(-1), 1.0)), np.inf)
        else:
            value = mn
    end = np.where(some, final.argmin(-1), -1)
    return dict(value=value, back=back, end=end)


def backtrack(back, end, n):
    """The states a(0 .. n - 1) of one pair from its back-pointers (T x S) and final state."""
    path = np.empty(n, dtype=np.int64)
    s = int(end)
    for t in range(n - 1, -1, -1):
        path[t] = s
        if t:
            s -= int(back[t, s])
    assert s == 0
    return path


def path_cost(c, path, log_move):
    """(sum of c along the path, -sum of log_move over its moves) in float64."""
    mv = np.diff(path)
    return float(sum(c[t, s] for t, s in enumerate(path))), float(-sum(log_move[m] for m in mv))


def brute_force(c, n, log_move, band=-1, marginal=False):
    """warp of one pair (c: T x S, n frames) by enumerating all 3^(n-1) move sequences."""
    S_ = c.shape[1]
    costs = []
    for moves in itertools.product(range(3), repeat=n - 1):
        if any(log_move[m] == NINF for m in moves):
            continue
        path = np.concatenate([[0], np.cumsum(moves)]).astype(np.int64)
        if path[-1] >= S_ or (band >= 0 and np.any(np.abs(path - np.arange(n)) > band)):
            continue
        tot = sum(c[t, s] for t, s in enumerate(path)) - sum(log_move[m] for m in moves)
        if not np.isnan(tot):
            costs.append(tot)
    if not costs:
        return np.inf
    costs = np.array(costs)
    if not marginal:
        return float(costs.min())
    m = costs.min()
    return float(m - np.log(np.exp(m - costs).sum())) if m < np.inf else np.inf


# ----------------------------------------------------------------------------
# the reference on the kernels' inputs
# ----------------------------------------------------------------------------
def cell_costs(batch_sizes, gt, mu, lv, o, y):
    """(e, Ae, off): B x P x T x S float64 emission terms, their units and the
    BCE terms of every cell (frames t >= len_b: 0).  mu / lv are S x P x F, o is
    S x P.  The quadratic form is expanded into three float64 matrix products;
    what that costs against the direct form is ~1e-13 of the unit."""
    bs = np.asarray(batch_sizes, dtype=np.int64)
    B, T = int(bs[0]), len(bs)
    gt, mu, lv, o, y = (S._np64(v) for v in (gt, mu, lv, o, y))
    S_, P, F = mu.shape
    off = np.concatenate([[0], np.cumsum(bs)])
    w = np.exp(-lv).reshape(S_ * P, F)
    m2 = mu.reshape(S_ * P, F)
    k_lv, k_abs = (LOG2PI + lv).sum(-1).reshape(-1), (LOG2PI + np.abs(lv)).sum(-1).reshape(-1)
    k_q = (m2 * m2 * w).sum(-1)
    e = np.zeros((B, P, T, S_))
    Ae, of = np.zeros_like(e), np.zeros_like(e)
    for t in range(T):
        n = int(bs[t])
        x = gt[off[t]:off[t] + n]
        q = (x * x) @ w.T - 2.0 * (x @ (m2 * w).T) + k_q[None]          # n x (S P)
        q = np.maximum(q, 0.0)                                           # NaN passes through
        e[:n, :, t, :] = (0.5 * (k_lv[None] + q)).reshape(n, S_, P).transpose(0, 2, 1)
        Ae[:n, :, t, :] = (0.5 * (k_abs[None] + q)).reshape(n, S_, P).transpose(0, 2, 1)
        v = o.T[None]                                                     # 1 x P x S
        of[:n, :, t, :] = np.maximum(v, 0.0) - v * y[off[t]:off[t] + n, None, None] + np.log1p(np.exp(-np.abs(v)))
    return e, Ae, of


def warp_reference(batch_sizes, gt, mu, lv, o, y, log_move, band=-1, marginal=False):
    """dict(value B x P (the mode asked for), viterbi B x P, paths {(b, p): states},
    em / off / move B x P (the Viterbi path's components), A B x P (its unit; 1
    where no alignment exists), c (the cost planes), lengths)."""
    lens = S.lengths_of(batch_sizes)
    e, Ae, of = cell_costs(batch_sizes, gt, mu, lv, o, y)
    c = e + of
    vit = dp(c, lens[:, None], log_move, band, False)
    B, P = vit["value"].shape
    em, off, move, A = (np.full((B, P), np.inf) for _ in range(4))
    paths = {}
    for b in range(B):
        for p in range(P):
            if vit["end"][b, p] < 0:
                A[b, p] = 1.0
                continue
            path = backtrack(vit["back"][b, p], vit["end"][b, p], int(lens[b]))
            tt = np.arange(len(path))
            mv = np.diff(path)
            paths[(b, p)] = path
            em[b, p], off[b, p] = e[b, p, tt, path].sum(), of[b, p, tt, path].sum()
            move[b, p] = -sum(log_move[m] for m in mv)
            A[b, p] = Ae[b, p, tt, path].sum() + np.abs(of[b, p, tt, path]).sum() + sum(abs(log_move[m]) for m in mv)
    value = dp(c, lens[:, None], log_move, band, True)["value"] if marginal else vit["value"]
    return dict(value=value, viterbi=vit["value"], paths=paths, em=em, off=off, move=move, A=A, c=c, lengths=lens)


# ----------------------------------------------------------------------------
# inputs of the C-ABI cases
# ----------------------------------------------------------------------------
def proto_steps(kind, T):
    """T_proto of a case: one state, shorter than the batch, longer, and past every state a path reaches."""
    return max(1, dict(one=1, short=T - 2, long=T + 3, double=2 * T + 1)[kind])


# (shape, F, P, row stride or 0 = F, T_proto kind, band, moves): a covering subset of the product, each run in
# both modes.  Every shape, P, F, stride, T_proto kind, band and move set occurs; the 37-frame shape (two frame
# blocks) meets every T_proto kind and band, and T_proto = 75 and 40 put it past one 32-step tile.
ABI_CASES = (
    ("b1t1", 1, 1, 0, "one", -1, "default"),
    ("b1t1", 65, 17, PAD_LD, "long", 0, "stepskip"),
    ("ties", 1, 33, 0, "double", -1, "default"),
    ("ties", 129, 17, PAD_LD, "short", 3, "staystep"),
    ("ties", 65, 1, 0, "long", 0, "identity"),
    ("ties", 65, 17, 0, "one", -1, "staystep"),
    ("b33t9", 129, 33, PAD_LD, "long", -1, "default"),
    ("b33t9", 65, 17, 0, "double", 3, "stepskip"),
    ("b33t9", 1, 1, 0, "short", 0, "default"),
    ("b33t9", 129, 1, 0, "one", -1, "stepskip"),
    ("b40t37", 129, 33, PAD_LD, "double", -1, "default"),
    ("b40t37", 65, 17, 0, "long", 3, "default"),
    ("b40t37", 129, 17, 0, "long", -1, "identity"),
    ("b40t37", 1, 33, 0, "short", -1, "staystep"),
    ("b40t37", 65, 1, PAD_LD, "double", 0, "stepskip"),
    ("b40t37", 65, 17, 0, "one", 3, "staystep"),
    ("b3t170", 1, 2, 0, "long", -1, "default"),
    ("b3t170", 65, 2, 0, "double", 3, "default"),
    ("b3t170", 1, 1, 0, "double", -1, "stepskip"),
    # a band whose lower edge meets a super-block boundary at the start of a frame block ((t0 - band) % 128 == 0,
    # t0 >= 128): the block's first super-block then starts at the edge, and its left predecessor at frame t0 - 1,
    # in the super-block that is no longer computed, is still inside the band (band 0: t0 = 128; band 32: t0 = 160)
    ("b3t170", 65, 2, 0, "long", 0, "default"),
    ("b3t170", 1, 2, 0, "long", 0, "identity"),
    ("b3t170", 65, 2, PAD_LD, "double", 32, "default"),
    ("b3t170", 1, 1, 0, "long", 32, "staystep"),
)


def case_id(case):
    shape, F, P, ld, kind, band, moves = case
    return f"{shape}-F{F}-P{P}-ld{ld or F}-{kind}-band{band}-{moves}"


@functools.lru_cache(maxsize=None)
def abi_inputs(shape, F, P, kind):
    """Random fp32 inputs of one (shape, F, P, T_proto kind), drawn as
    pairwise_cases.abi_inputs draws them: mu N(0, 1), lv U[-6, 2], every
    segment's frames around the steps of one random prototype taken at a random
    monotone warp, offset logits U[-8, 8], 0/1 targets.  Shared, never modified."""
    lengths = ABI_SHAPES[shape]
    bs = S.batch_sizes_of(lengths)
    T, B, L = len(bs), len(lengths), int(bs.sum())
    S_ = proto_steps(kind, T)
    g = torch.Generator().manual_seed(100000 * P + 1000 * B + 10 * F + S_)
    mu = torch.randn(S_, P, F, generator=g)
    lv = torch.rand(S_, P, F, generator=g) * 8.0 - 6.0
    own = torch.randint(0, P, (B,), generator=g)
    t_of, b_of = torch.from_numpy(PW.step_of_rows(bs)), torch.from_numpy(S.segment_of_rows(bs))
    speed = torch.rand(B, generator=g) * 1.5 + 0.5
    s_of = torch.clamp((t_of.double() * speed[b_of].double()).long(), max=S_ - 1)
    m, v = mu[s_of, own[b_of]], lv[s_of, own[b_of]]
    gt = m + torch.randn(L, F, generator=g) * torch.exp(0.5 * v) * 1.5
    o = torch.rand(S_, P, generator=g) * 16.0 - 8.0
    y = (torch.rand(L, generator=g) < 0.3).float()
    return dict(lengths=lengths, batch_sizes=bs, T=T, B=B, L=L, F=F, P=P, S=S_, gt=gt, mu=mu, lv=lv, o=o, y=y)


@functools.lru_cache(maxsize=None)
def abi_reference(shape, F, P, kind, band, moves, marginal):
    d = abi_inputs(shape, F, P, kind)
    return warp_reference(d["batch_sizes"], d["gt"], d["mu"], d["lv"], d["o"], d["y"], MOVES[moves], band, marginal)


# ----------------------------------------------------------------------------
# planted alignments
# ----------------------------------------------------------------------------
PLANTS = dict(half=[t // 2 for t in range(20)],
              double=[2 * t for t in range(12)],
              mixed=[0, 0, 1, 2, 4, 6, 7, 7, 7, 8, 10, 11])
PLANT_P, PLANT_S, PLANT_F, PLANT_CAT = 5, 24, 9, 3


@functools.lru_cache(maxsize=None)
def planted(name):
    """One segment that follows prototype 3 at the planted states: mu N(0, 1),
    lv = -2, offset logits -8 except +8 at the planted end state, frames = the
    prototype at the planted states + 0.05 N(0, 1), target 1 on the last frame."""
    a = PLANTS[name]
    n = len(a)
    g = torch.Generator().manual_seed(4242 + n)
    mu = torch.randn(PLANT_S, PLANT_P, PLANT_F, generator=g)
    lv = torch.full((PLANT_S, PLANT_P, PLANT_F), -2.0)
    o = torch.full((PLANT_S, PLANT_P), -8.0)
    o[a[-1], :] = 8.0
    gt = mu[torch.tensor(a), PLANT_CAT] + 0.05 * torch.randn(n, PLANT_F, generator=g)
    y = torch.zeros(n)
    y[-1] = 1.0
    bs = np.ones(n, dtype=np.int64)
    return dict(batch_sizes=bs, gt=gt, mu=mu, lv=lv, o=o, y=y, plant=np.array(a), T=n, B=1, L=n, F=PLANT_F,
                P=PLANT_P, S=PLANT_S)


EDGE_BAND, EDGE_FRAMES, EDGE_S, EDGE_P, EDGE_F, EDGE_CAT = 32, 170, 150, 2, 9, 1


@functools.lru_cache(maxsize=None)
def edge_planted():
    """One 170-frame segment planted ALONG the lower edge of a band of 32:
    a(t) = max(0, t - 32) on prototype 1, drawn as ``planted`` draws.  At frame
    160, where a frame block starts, the edge sits on state 128, a super-block
    boundary; the path comes from (159, 127), in the super-block below, which
    frame 160's block no longer computes."""
    a = [max(0, t - EDGE_BAND) for t in range(EDGE_FRAMES)]
    g = torch.Generator().manual_seed(777)
    mu = torch.randn(EDGE_S, EDGE_P, EDGE_F, generator=g)
    lv = torch.full((EDGE_S, EDGE_P, EDGE_F), -2.0)
    o = torch.full((EDGE_S, EDGE_P), -8.0)
    o[a[-1], :] = 8.0
    gt = mu[torch.tensor(a), EDGE_CAT] + 0.05 * torch.randn(EDGE_FRAMES, EDGE_F, generator=g)
    y = torch.zeros(EDGE_FRAMES)
    y[-1] = 1.0
    return dict(batch_sizes=np.ones(EDGE_FRAMES, dtype=np.int64), gt=gt, mu=mu, lv=lv, o=o, y=y, plant=np.array(a),
                T=EDGE_FRAMES, B=1, L=EDGE_FRAMES, F=EDGE_F, P=EDGE_P, S=EDGE_S)


def dump(name, rows):
    """The figures a GPU test observed (ABCD_PARITY_DUMP=<dir>, as edge_cases.dump_observed)."""
    E.dump_observed("warp_" + name, rows)


def assemble(dump_dir, out_path, date, parent_commit):
    """profiles/warp_errors.json from a run of tests/test_gpu_warp.py with
    ABCD_PARITY_DUMP=<dump_dir>."""
    import glob
    import json
    rows = {}
    for kind in ("abi", "path", "e2e"):
        rows[kind] = []
        for path in sorted(glob.glob(os.path.join(dump_dir, f"warp_{kind}_*.json"))):
            with open(path) as f:
                rows[kind] += json.load(f)
    ident = [r for r in rows["abi"] if "vs_pairwise" in r]
    worst = dict(abi_warp=max(r["warp"] for r in rows["abi"]),
                 abi_vs_pairwise_over_bar=max((r["vs_pairwise"] / (2 * cross_bar(r["F"])) for r in ident), default=None),
                 path_cost_under_optimum=max((r["under_optimum"] for r in rows["path"]), default=None),
                 path_components=max((r["components"] for r in rows["path"]), default=None),
                 e2e_vs_score_against_over_bar=max((r["vs_score_against_over_bar"] for r in rows["e2e"]), default=None))
    doc = dict(what="figures observed by tests/test_gpu_warp.py (ABCD_PARITY_DUMP) on one MI355X, in units of A[b,p]; "
                    "units and bars: tests/warp_cases.py", date=date, parent_commit=parent_commit,
               bars=dict(warp=BAR, vs_pairwise="2 (F + 4) 2^-23 A[b,p]", path=BAR, planted="equality",
                         determinism="bit equality"),
               worst=worst, **rows)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


if __name__ == "__main__":  # python tests/warp_cases.py <dump directory> <out.json> <date> <parent commit>
    print(assemble(*sys.argv[1:5])["worst"])
