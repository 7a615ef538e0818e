"""The category-sequence HMM on the GPU: ``abcd_chain_posterior`` (both forms,
taken from ``abcd_chain_plan``) against the float64 oracle of
``chain_cases.py`` on every generated case, its determinism, exclusions and
NULL outputs; ``TransitionModel`` against ``ops.pair_posterior`` and the
oracle's EM; ``sequence.py`` on the toy data.

Outputs are pre-filled with NaN, so an unwritten element shows.  The bars come
from the float32 oracle's own error on the same inputs (``chain_cases.bars``).
Every observed figure is printed (``-rA``) and kept with ``ABCD_PARITY_DUMP``
(profiles/chain_errors.json)."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import chain_cases as C
import pairwise_cases as PW
from test_gpu_score import ANN, CKPT, TOY, _bits

pytestmark = pytest.mark.gpu
NAN = float("nan")
GROUPS = {"ev": C.WANT_EVIDENCE, "gamma": C.WANT_GAMMA, "path": C.WANT_PATH, "counts": C.WANT_COUNTS}


def chain_call(score, seq_off, log_trans, log_init, want=("ev", "gamma", "path", "counts"), K=None):
    """abcd_chain_posterior through ctypes on (possibly padded) device tensors:
    dict of the NaN-prefilled outputs that were asked for."""
    from modules import _native as N
    lib = N.lib()
    dev = "cuda"
    K = int(log_init.numel()) if K is None else K
    sc, lt, li = score.to(dev), log_trans.to(dev), log_init.to(dev)
    so = torch.as_tensor(seq_off, dtype=torch.int64).contiguous()
    n, S = int(sc.shape[0]), int(so.numel()) - 1
    bits = sum(GROUPS[w] for w in want)
    nbytes = lib.abcd_chain_workspace_bytes(n, S, K, bits)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    f64 = dict(dtype=torch.float64, device=dev)
    out = {}
    if "ev" in want:
        out["log_evidence"] = torch.full((S,), NAN, **f64)
    if "gamma" in want:
        out["gamma"] = torch.full((n, K + 2), NAN, device=dev)
    if "path" in want:
        out["path"] = torch.full((n,), -7, dtype=torch.int32, device=dev)
        out["path_score"] = torch.full((S,), NAN, **f64)
    if "counts" in want:
        out["trans_counts"] = torch.full((K, K), NAN, **f64)
        out["init_counts"] = torch.full((K,), NAN, **f64)
    p = lambda k: N.ptr(out.get(k))  # noqa: E731
    rc = lib.abcd_chain_posterior(N.ptr(sc), sc.stride(0), n, K, so.data_ptr(), S, N.ptr(lt), lt.stride(0), N.ptr(li),
                                  p("log_evidence"), p("gamma"), K + 2, p("path"), p("path_score"), p("trans_counts"),
                                  p("init_counts"), N.ptr(ws), ws.numel(), N.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if "gamma" in out:
        assert torch.isnan(out["gamma"][:, K:]).all()       # the padding is not written
        out["gamma"] = out["gamma"][:, :K]
    return out


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("K,kind", C.case_ids())
def test_chain_against_the_float64_oracle(K, kind):
    c = C.case(K, kind)
    ref, bar = c["ref"], C.bars(c)
    assert C.plan(K, 1)[0] == (K < C.first_streaming_k())
    got = chain_call(c["score"], c["seq_off"], c["log_trans"], c["log_init"])
    ev, gamma, path, ps = (_np(got[k]) for k in ("log_evidence", "gamma", "path", "path_score"))
    tc, ic = _np(got["trans_counts"]), _np(got["init_counts"])
    lens = np.diff(c["seq_off"].numpy())
    e_ev, e_ps = C.rel_err(ev, ref["log_evidence"]), C.rel_err(ps, ref["path_score"])
    e_g = float(np.abs(gamma - ref["gamma"]).max()) if gamma.size else 0.0
    e_c = max(float(np.abs(tc - ref["trans_counts"]).max()), float(np.abs(ic - ref["init_counts"]).max()))
    rows_sum = float(np.abs(gamma.sum(1) - 1.0).max()) if gamma.size else 0.0
    # Viterbi: the returned path scored in float64 reaches the optimum; decided sequences match exactly
    lj = C.path_log_joint(path, c["score"].numpy(), c["seq_off"].numpy(), c["log_trans"].numpy(),
                          c["log_init"].numpy())
    e_opt = C.rel_err(lj, ref["path_score"])
    decided = ref["decided"]
    row_dec = np.repeat(decided, lens)
    row = dict(K=K, kind=kind, S=len(lens), N=int(lens.sum()), resident=C.plan(K, 1)[0], evidence=e_ev,
               evidence_bar=bar["evidence"], path_score=e_ps, path_score_bar=bar["path_score"], gamma=e_g,
               gamma_bar=bar["gamma"], counts=e_c, counts_bar=bar["counts"], path_optimum=e_opt,
               gamma_row_sum=rows_sum, undecided=int((~decided).sum()), e32=bar["e32"])
    print(row)
    C.dump(f"k{K}_{kind}", row)
    assert e_ev <= bar["evidence"] and e_ps <= bar["path_score"]
    assert e_g <= bar["gamma"] and e_c <= bar["counts"]
    assert rows_sum <= 1e-5
    assert e_opt <= bar["path_score"]
    assert (path[row_dec] == ref["path"][row_dec]).all()
    assert ((path >= 0) & (path < K)).all()


def test_two_calls_and_a_sequence_alone_agree_bit_for_bit():
    for K in (128, C.first_streaming_k()):
        c = C.case(K, "many")
        a = chain_call(c["score"], c["seq_off"], c["log_trans"], c["log_init"])
        b = chain_call(c["score"], c["seq_off"], c["log_trans"], c["log_init"])
        for k in a:
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype != torch.float64 else a[k].view(torch.int64),
                               b[k].view(torch.int32) if b[k].dtype != torch.float64 else b[k].view(torch.int64)), k
        off = c["seq_off"].numpy()
        lens = np.diff(off)
        for s in (int(np.argmax(lens)), int(np.flatnonzero(lens == 17)[0]), int(np.flatnonzero(lens == 1)[0])):
            r0, r1 = int(off[s]), int(off[s + 1])
            one = chain_call(c["score"][r0:r1], [0, r1 - r0], c["log_trans"], c["log_init"], want=("ev", "gamma", "path"))
            assert torch.equal(_bits(one["gamma"].contiguous()), _bits(a["gamma"][r0:r1].contiguous()))
            assert torch.equal(one["path"], a["path"][r0:r1])
            assert torch.equal(one["log_evidence"].view(torch.int64), a["log_evidence"][s:s + 1].view(torch.int64))
            assert torch.equal(one["path_score"].view(torch.int64), a["path_score"][s:s + 1].view(torch.int64))


def test_exclusions():
    inf = float("inf")
    K = 4
    g = np.random.default_rng(3)
    trans, init = C.draw_chain(K, g, zeros=False)
    lt, li = torch.tensor(np.log(trans), dtype=torch.float32), torch.tensor(np.log(init), dtype=torch.float32)
    sc = torch.tensor(-3.0 * g.random((9, K)), dtype=torch.float32)
    sc[1] = NAN                              # sequence 0 (rows 0-2): an all-excluded row
    sc[4, 1], sc[4, 2] = NAN, inf            # sequence 1 (rows 3-5): single excluded entries
    off = [0, 3, 6, 6, 9]                    # sequence 2 is empty, sequence 3 (rows 6-8) is clean
    ref = C.oracle(sc.numpy(), off, lt.numpy(), li.numpy())
    got = chain_call(sc, off, lt, li)
    ev, ps = _np(got["log_evidence"]), _np(got["path_score"])
    assert ev[0] == -inf and ps[0] == -inf and (_np(got["path"])[:3] == -1).all() and (_np(got["gamma"])[:3] == 0).all()
    assert ev[2] == 0.0 and np.isnan(ps[2])
    assert (_np(got["gamma"])[4, 1:3] == 0).all()
    assert C.rel_err(ev, ref["log_evidence"]) <= 1e-6 and C.rel_err(ps, ref["path_score"]) <= 1e-6
    assert np.abs(_np(got["gamma"]) - ref["gamma"]).max() <= 1e-6
    assert (_np(got["path"]) == ref["path"]).all()
    assert np.abs(_np(got["trans_counts"]) - ref["trans_counts"]).max() <= 1e-5   # the dead sequence adds nothing
    assert np.abs(_np(got["init_counts"]) - ref["init_counts"]).max() <= 1e-6
    assert abs(_np(got["init_counts"]).sum() - 2.0) <= 1e-6
    # a structural zero that kills a sequence: state 0 is forced at row 0, state 1 at row 1, and 0 -> 1 is impossible
    lt2 = lt.clone()
    lt2[0, 1] = -inf
    sc2 = torch.full((2, K), -inf)
    sc2[0, 0], sc2[1, 1] = 0.0, 0.0
    dead = chain_call(sc2, [0, 2], lt2, li)
    assert _np(dead["log_evidence"])[0] == -inf and (_np(dead["path"]) == -1).all()
    assert (_np(dead["gamma"]) == 0).all() and (_np(dead["trans_counts"]) == 0).all()
    assert (_np(dead["init_counts"]) == 0).all() and _np(dead["path_score"])[0] == -inf
    only_path = chain_call(sc2, [0, 2], lt2, li, want=("path",))       # found without a forward pass too
    assert (_np(only_path["path"]) == -1).all() and _np(only_path["path_score"])[0] == -inf
    # the state 90 nats behind in its row is the only one the transitions allow: it carries the chain
    for K2 in (5, C.first_streaming_k()):
        lt3 = torch.full((K2, K2), -inf)
        lt3[:, 2] = 0.0                                                    # every state goes to state 2
        li3 = torch.full((K2,), -float(np.log(K2)))
        sc3 = torch.zeros(3, K2)
        sc3[1, 2] = -90.0
        sc3[2, 2] = -90.0
        ref3 = C.oracle(sc3.numpy(), [0, 3], lt3.numpy(), li3.numpy())
        got3 = chain_call(sc3, [0, 3], lt3, li3)
        assert abs(_np(got3["log_evidence"])[0] - ref3["log_evidence"][0]) <= 2.0 ** -22 * 180
        assert abs(ref3["log_evidence"][0] + 180.0) < 1e-6       # log_init = -log K in fp32 sums to 1 within 2^-24 K
        # alpha + beta and log Z are sums of magnitude 180 here: an fp32 rounding of such a value is 2^-17, and a
        # probability moves by that much relative; a few of them, with the project's factor of 4
        tol = 4 * 2.0 ** -17
        assert _np(got3["path"])[1:].tolist() == [2, 2] and np.abs(_np(got3["gamma"]) - ref3["gamma"]).max() <= tol
        assert abs(_np(got3["trans_counts"])[:, 2].sum() - 2.0) <= 2 * tol


def test_null_outputs_leave_the_others_unchanged():
    for K in (65, C.first_streaming_k()):
        c = C.case(K, "three")
        full = chain_call(c["score"], c["seq_off"], c["log_trans"], c["log_init"])
        keys = {"ev": ("log_evidence",), "gamma": ("gamma",), "path": ("path", "path_score"),
                "counts": ("trans_counts", "init_counts")}
        for g, ks in keys.items():
            one = chain_call(c["score"], c["seq_off"], c["log_trans"], c["log_init"], want=(g,))
            for k in ks:
                a, b = one[k].contiguous(), full[k].contiguous()
                w = torch.int64 if a.dtype == torch.float64 else torch.int32
                assert torch.equal(a.view(w), b.view(w)), (K, k)


def test_transition_model_reproduces_pair_posterior():
    from modules import ops
    from modules.sequence import TransitionModel
    rows = []
    for B, P in ((33, 16), (33, 130), (5, 65)):
        c = PW.posterior_inputs(B, P)
        em, off, lw = (c[k].cuda() for k in ("em", "off", "lw"))
        ref = c["ref"]
        score, row_off = ops.chain_scores(em, off)
        assert score.dtype == torch.float32 and row_off.dtype == torch.float64 and float(score.max(1).values.abs().max()) == 0
        model = TransitionModel.from_log_weight(lw)
        seq_off = [0, 1, B // 2, B]
        post = model.posterior(score, seq_off)
        path, _ = model.viterbi(score, seq_off)
        ev_p, best_p, _, resp_p = ops.pair_posterior(em, off, lw)
        # the same inputs through the float64 / float32 oracle: the bars of this case
        sc_np, lt_np, li_np = score.cpu().numpy(), model.log_trans.cpu().numpy(), model.log_init.cpu().numpy()
        r64 = C.oracle(sc_np, seq_off, lt_np, li_np)
        r32 = C.oracle(sc_np, seq_off, lt_np, li_np, dtype=np.float32)
        # e32: the float32 oracle on the same fp32 inputs against this test's reference (resp, from the unrounded
        # NLLs and weights in float64), so it carries the rounding of the inputs as the kernel's figure does
        g_bar = C.ORDER_FACTOR * float(np.abs(r32["gamma"] - ref["resp"]).max())
        e_g = float(np.abs(post["gamma"].cpu().numpy() - ref["resp"]).max())
        # pair evidence = chain evidence + the row offsets + logsumexp(lw) per row
        lse_lw = float(torch.logsumexp(lw.double(), 0))
        rest = float(row_off.sum()) + B * lse_lw
        total = float(post["log_evidence"].sum()) + rest
        want = float(ref["log_evidence"].sum())
        e32_ev = abs(float(r32["log_evidence"].astype(np.float64).sum()) + rest - want) / abs(want)
        ev_bar = max(C.CAST_FLOOR, C.ORDER_FACTOR * e32_ev)
        rows.append(dict(B=B, P=P, gamma=e_g, gamma_bar=g_bar, evidence=abs(total - want) / abs(want),
                         evidence_bar=ev_bar, gamma_vs_kernel=float((post["gamma"] - resp_p).abs().max()),
                         gamma_f64_oracle=float(np.abs(r64["gamma"] - ref["resp"]).max())))
        print(rows[-1])
        assert e_g <= g_bar
        decided = PW.top_two_gap(ref["s"]) >= 0.5
        assert (path.cpu().numpy()[decided] == ref["best"][decided]).all()
        assert abs(total - want) <= ev_bar * abs(want)
    C.dump("pair_posterior", rows)


def test_fit_climbs_and_matches_the_oracle():
    from modules.sequence import TransitionModel
    c = C.case(5, "many")
    K = 5
    score = c["score"][:, :K].contiguous().cuda()
    model = TransitionModel(K).cuda()
    objs = model.fit(score, c["seq_off"], n_iter=5, pseudo_count=0.2)
    got = np.array([model.initial_objective] + objs)
    u = np.full((K, K), -np.log(K), dtype=np.float32)
    want = C.em_reference(c["score"].numpy(), c["seq_off"].numpy(), u, u[0], 5, 0.2)
    bar = C.bars(c)["evidence"]
    print(dict(objective=got.tolist(), oracle=want.tolist(), bar=bar, rel=float(np.abs(got / want - 1).max())))
    assert len(objs) == 5
    assert (np.diff(got) >= -bar * np.abs(got[1:])).all()
    assert (np.abs(got - want) <= bar * np.abs(want)).all()
    assert got[-1] > got[0]
    tc, ic = model.last_counts
    assert abs(float(tc.sum()) - float((np.maximum(np.diff(c["seq_off"].numpy()), 1) - 1).sum())) < 1e-3
    assert torch.allclose(model.log_trans.double().exp().sum(1), torch.ones(K, dtype=torch.float64, device="cuda"),
                          atol=1e-5)


def test_sequence_cli_on_toy_data(tmp_path):
    import classify
    import sequence
    base = [CKPT, TOY, ANN, "1.0", "-b", "4"]
    d = os.path.join(str(tmp_path), "s")
    assert sequence.main(base + ["-S", d, "--em_iterations", "2"]) == d
    cls = os.path.join(str(tmp_path), "classified.csv")
    classify.main(base + ["-S", cls])
    seg = pd.read_csv(os.path.join(d, "sequenced.csv"))
    tr = pd.read_csv(os.path.join(d, "transitions.csv"))
    sq = pd.read_csv(os.path.join(d, "sequences.csv"))
    ann = pd.read_csv(ANN)
    n = len(ann)
    assert list(seg.columns) == list(sequence.COLUMNS) + list(ann.columns)
    assert list(tr.columns) == list(sequence.TRANSITION_COLUMNS) and list(sq.columns) == list(sequence.SEQUENCE_COLUMNS)
    assert sorted(seg["data_ix"].tolist()) == list(range(n)) and sq["length"].sum() == n
    K = int(np.sqrt(len(tr)))
    assert K * K == len(tr) and np.abs(tr.groupby("from_ix")["probability"].sum() - 1.0).max() < 1e-5
    assert abs(tr["expected_count"].sum() - (n - len(sq))) < 1e-3 * max(n, 1)
    assert (seg["changed"] == (seg["viterbi_category_ix"] != seg["decoder_category_ix"]).astype(int)).all()
    assert (seg.groupby("sequence_ix")["position"].apply(list).map(lambda p: p == list(range(len(p))))).all()
    # the context-free evidence is classify.py's, summed over the sequence
    cf = pd.read_csv(cls).set_index("data_ix")["log_evidence"]
    want = seg.assign(ev=cf[seg["data_ix"]].to_numpy()).groupby("sequence_ix")["ev"].sum()
    got = sq.set_index("sequence_ix")["context_free_log_evidence"]
    assert (np.abs(got - want[got.index]) <= 1e-6 * np.abs(want[got.index])).all()
    assert (seg["decoder_category_ix"].to_numpy() ==
            pd.read_csv(cls).set_index("data_ix")["decoder_category_ix"][seg["data_ix"]].to_numpy()).all()
    # without EM the chain is the context-free model: no label changes, and the evidence is the context-free one
    d0 = os.path.join(str(tmp_path), "s0")
    sequence.main(base + ["-S", d0, "--em_iterations", "0"])
    seg0, sq0 = pd.read_csv(os.path.join(d0, "sequenced.csv")), pd.read_csv(os.path.join(d0, "sequences.csv"))
    assert (seg0["changed"] == 0).all()
    assert (np.abs(sq0["log_evidence"] - sq0["context_free_log_evidence"])
            <= 1e-6 * np.abs(sq0["context_free_log_evidence"])).all()
    # a rerun keeps the earlier tables, and a saved matrix can be loaded instead of fitted
    sequence.main(base + ["-S", d0, "--em_iterations", "0"])
    assert sorted(os.listdir(d0)) == sorted(f + e for f in ("sequenced.csv", "transitions.csv", "sequences.csv")
                                            for e in ("", ".prev"))
    d1 = os.path.join(str(tmp_path), "s1")
    sequence.main(base + ["-S", d1, "--transitions", os.path.join(d, "transitions.csv")])
    tr1 = pd.read_csv(os.path.join(d1, "transitions.csv"))
    assert np.abs(tr1["probability"] - tr["probability"]).max() <= 1e-6 and len(pd.read_csv(
        os.path.join(d1, "sequenced.csv"))) == n
